"""Sinusoid exposure bins on the GPU (run with -m gpu): wagg_exposure_reduce_* through engine.exposure_reduce against the NumPy
restatement of tests/exposure_ref.py (shift and edge in the element type, then fp64 with np.arccos), the exact cases bit for
bit, the tangency probes, band skipping, the laws of the bins, the degree-day ladder kernel, and snyder_exposure_aggregate.

THE BOUND of every parity check: |got - want| <= tol * D, D the cell's counted days of the period (listed, in season, no NaN
in either field), tol = 1e-4 (fp32) / 1e-6 (fp64), the project's tolerances.  The largest observed ratio to that bound is
printed by every test that measures one."""
import numpy as np
import pytest

from tests import exposure_ref as ER
from tests.test_gpu_periods import _Case, _psum
from tests.test_gpu_seasons import KELVIN, _mask_TG, _mixed_cells, _pack, _seasons_for, plan_kind  # noqa: F401
from tests.test_seasons_host import ref_mask

pytestmark = pytest.mark.gpu

INF = float("inf")
TOL = {np.float32: 1e-4, np.float64: 1e-6}
T0 = 41
RB = np.array([0, 12, 12, 32, 42])                                  # four periods of unequal length, the second empty
ROWS = np.concatenate([np.arange(12), np.arange(12, 21), [20], np.arange(21, 31), np.arange(40, 30, -1)])      # row 20 twice
DOY = np.arange(100, 100 + T0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _tdt(torch, dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


def _dev(torch, host, pad=0):
    """the (T, n) host array as a device tensor of row stride n + pad"""
    T, n = host.shape
    buf = torch.zeros((T, n + pad), dtype=_tdt(torch, host.dtype.type), device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return buf[:, :n]


def _edges(m):
    if m == 2:
        return [10.0, 25.0]
    return [-INF] + [float(v) for v in np.linspace(-2.0, 40.0, m - 2)] + [INF]


def _kelvin_pair(seed, T, n, dtype):
    """Kelvin tasmin / tasmax whose Celsius values spread over -6 .. 52, with NaN in either field alone and in both"""
    rng = np.random.default_rng(seed)
    lo = (273.15 + rng.uniform(-6.0, 36.0, (T, n))).astype(dtype)
    hi = (lo + rng.uniform(0.0, 16.0, (T, n)).astype(dtype)).astype(dtype)
    flat = rng.random((T, n)) < 0.05
    hi[flat] = lo[flat]                                             # days with tasmin == tasmax
    lo[1, 0] = np.nan
    if n > 2:
        hi[2, n // 2] = np.nan
        lo[3, n - 1] = hi[3, n - 1] = np.nan
    return lo, hi


def _windows(n):
    z1, z2 = _mixed_cells(n, DOY)                                   # open, null, empty (no listed day), single day, plain, wrapping
    return _pack(z1, z2), np.nan_to_num(ref_mask(z1, z2, DOY), nan=0.0).T


def _check(got, want, D, tol, what):
    got = got.double().cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err, bound = np.abs(got - want), tol * D[None]
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, "%r: %d values beyond tol * D, first at (bin, period, cell) %r: got %r, want %r, D %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], D[tuple(bad[0][1:])])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, err / bound, 0.0))) if err.size else 0.0
    return got, ratio


# which kernel a case runs (rowlist_geometry: 16-byte pieces only if the row stride is a multiple of the piece, 4 fp32 / 2 fp64 cells):
#   stride n, n in 1, 3, 5, 255, 1025 (odd): cell by cell in both types;  (4, 0): pieces, one whole piece
#   (5, 3) stride 8, (255, 1) stride 256, (1025, 3) stride 1028: pieces in both types, the last piece partial (1, 3 and 1 cells
#   in fp32; 1 cell in fp64), one block short of full and one past a block
#   (1025, 2) stride 1027: a row stride larger than n that is no multiple of 4 (nor of 2): cell by cell with ldx > n
CASES_N = [(1, 0), (3, 0), (4, 0), (5, 0), (5, 3), (255, 0), (255, 1), (1025, 0), (1025, 2), (1025, 3)]


def _is_wide(n, pad, dtype):
    return (n + pad) % (16 // np.dtype(dtype).itemsize) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,pad", CASES_N)
def test_bins_match_the_restatement(torch_cuda, dtype, n, pad):
    """Kelvin fields with offset -273.15 and 2, 3, G + 1, G + 2, 17 and 65 edges in degrees C, with and without a season (null,
    empty, single-day, plain and wrapping windows), with and without the workspace, on four periods of unequal length (one empty,
    one row listed twice, one list descending): n around the 16-byte piece, one short of a block, one past a block; contiguous
    rows (an odd stride: the cell-by-cell kernel), padded rows whose stride is a multiple of 4 (the 16-byte kernel with a
    partial last piece) and a padded row whose stride 1027 is no multiple of 4 (the cell-by-cell kernel with ldx > n) -- see
    CASES_N.  Every value within tol * D of the restatement; status 0; the
    empty period, null and empty windows and days with NaN in either field count exactly 0.  The laws on the device results:
    with both ends open the bins sum to D within n_bins * eps * D; every bin is at least -tol * D; merging two adjacent bins
    gives the wider bin within tol * D."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    G, tol, eps = _lib.EXPOSURE_GROUP, TOL[dtype], float(np.finfo(dtype).eps)
    lo, hi = _kelvin_pair(1000 + n, T0, n, dtype)
    Xlo, Xhi = _dev(torch, lo, pad), _dev(torch, hi, pad)
    assert Xlo.stride(0) == n + pad and Xlo.data_ptr() % 16 == 0
    assert _is_wide(n, pad, dtype) == ((n, pad) in ((4, 0), (5, 3), (255, 1), (1025, 3)))
    win, m01 = _windows(n)
    worst = 0.0
    for season, m in ((True, m01), (False, np.ones_like(m01))):
        kw = {"doy": DOY, "windows": win} if season else {}
        D = ER.counted_days(lo, hi, RB, ROWS, m)
        for count in (2, 3, G + 1, G + 2, 17, 65):
            edges = _edges(count)
            want = ER.exposure_bins(lo, hi, KELVIN, edges, RB, ROWS, m)
            for workspace in (True, False):
                what = (n, pad, season, count, workspace)
                got, st = engine.exposure_reduce(Xlo, Xhi, RB, ROWS, KELVIN, edges, workspace=workspace, **kw)
                assert got.dtype == _tdt(torch, dtype) and tuple(got.shape) == (count - 1, 4, n) and int(st.item()) == 0, what
                g, ratio = _check(got, want, D, tol, what)
                worst = max(worst, ratio)
                assert (g[:, 1] == 0).all(), what                                   # the empty period
                assert (g[:, :, D.sum(0) == 0] == 0).all(), what                    # null / empty windows, all-NaN cells: exactly 0
                assert (g >= -tol * D[None]).all(), what
                if count > 2:
                    assert (np.abs(g.sum(0) - D) <= (count - 1) * eps * D).all(), what
            if count == 17:
                merged, _ = engine.exposure_reduce(Xlo, Xhi, RB, ROWS, KELVIN, edges[:5] + edges[6:], **kw)
                mg = merged.double().cpu().numpy()
                assert (np.abs(mg[4] - (g[4] + g[5])) <= tol * D).all() and (np.abs(mg[5:] - g[6:]) <= tol * D[None]).all(), what
    print("exposure bins %s n=%d pad=%d: largest |got - want| / (tol * D) = %.3g" % (np.dtype(dtype).name, n, pad, worst))


PADS = pytest.mark.parametrize("wide", [False, True], ids=["cells", "pieces"])


def _pad_for(n, wide):
    """the row padding that makes the stride n + pad a multiple of 4 (the 16-byte kernel in both types) or leaves it odd"""
    pad = (-n) % 4 if wide else (0 if n % 2 else 1)
    assert ((n + pad) % 4 == 0) if wide else ((n + pad) % 2 == 1)
    return pad


@PADS
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_list_long_enough_to_be_split(torch_cuda, dtype, wide):
    """T = 70 rows in one period on 63 cells: too few blocks, so with the workspace the list is cut into parts and the fp64
    partial sums are added by the finish kernel; without it one block walks the list.  Both within the bound, on the
    cell-by-cell kernel (stride 63) and on the 16-byte kernel (stride 64)."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    T, n = 70, 63
    assert _lib.load().wagg_exposure_work_bytes(n, 1, T, 18) > 0                    # (the rule does split this call)
    lo, hi = _kelvin_pair(7, T, n, dtype)
    rb, rows = np.array([0, T]), np.arange(T)
    edges = _edges(18)
    D = ER.counted_days(lo, hi, rb, rows)
    want = ER.exposure_bins(lo, hi, KELVIN, edges, rb, rows)
    for workspace in (True, False):
        pad = _pad_for(n, wide)
        got, st = engine.exposure_reduce(_dev(torch, lo, pad), _dev(torch, hi, pad), rb, rows, KELVIN, edges, workspace=workspace)
        _, ratio = _check(got, want, D, TOL[dtype], ("split", workspace))
        assert int(st.item()) == 0
        print("exposure bins %s, T = 70 in one period, workspace=%r: ratio to the bound %.3g" % (np.dtype(dtype).name, workspace, ratio))


@PADS
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_cases_bit_for_bit(torch_cuda, dtype, wide):
    """Days wholly below or above every edge, tasmin == edge (1), tasmax == edge (0), NaN in either field alone (0 at every
    edge, -inf included): the sums are whole numbers of days, exactly.  tasmin == tasmax with offset 0: the planes are those of
    engine.bin_days_reduce of the same field and edges (edges that are values of the element type).  Out-of-season +-inf
    changes neither a bit nor the status word; in season it sets bit 0.  All of it on the cell-by-cell kernel (odd row stride)
    and on the 16-byte kernel (rows padded to a multiple of 4 cells)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    dev = lambda host: _dev(torch, host, _pad_for(host.shape[1], wide))       # rows padded to the kernel asked for
    T, n = 12, 9
    rng = np.random.default_rng(3)
    lo = rng.uniform(11.0, 14.0, (T, n)).astype(dtype)
    hi = (lo + dtype(4.0)).astype(dtype)
    lo[:, 0], hi[:, 0] = rng.uniform(-9.0, -5.0, T), rng.uniform(-4.0, -1.0, T)          # wholly below every edge
    lo[:, 1], hi[:, 1] = rng.uniform(31.0, 34.0, T), rng.uniform(35.0, 39.0, T)          # wholly above
    lo[:, 2], hi[:, 2] = 10.0, rng.uniform(12.0, 19.0, T)                                # tasmin on the edge 10
    lo[:, 3], hi[:, 3] = rng.uniform(11.0, 15.0, T), 20.0                                # tasmax on the edge 20
    lo[:, 4] = np.nan
    hi[:, 5] = np.nan
    rb, rows = np.array([0, 5, T]), np.arange(T)
    days = np.array([5.0, 7.0])
    Xlo, Xhi = dev(lo), dev(hi)
    got, st = engine.exposure_reduce(Xlo, Xhi, rb, rows, 0.0, [0.0, 10.0, 20.0, 30.0])
    g = got.double().cpu().numpy()
    assert int(st.item()) == 0
    zero = np.zeros(2)
    for j in (0, 1, 4, 5):
        assert all(np.array_equal(g[k, :, j], zero) for k in range(3)), j
    assert np.array_equal(g[0, :, 2], zero) and np.array_equal(g[1, :, 2], days) and np.array_equal(g[2, :, 2], zero)
    assert np.array_equal(g[0, :, 3], zero) and np.array_equal(g[1, :, 3], days) and np.array_equal(g[2, :, 3], zero)
    got, st = engine.exposure_reduce(Xlo, Xhi, rb, rows, 0.0, [-INF, 0.0, 10.0, 20.0, 30.0, INF])
    g = got.double().cpu().numpy()
    assert np.array_equal(g[0, :, 0], days) and np.array_equal(g[1:, :, 0].sum(0), zero)
    assert np.array_equal(g[4, :, 1], days) and np.array_equal(g[:4, :, 1].sum(0), zero)
    assert (g[:, :, 4] == 0).all() and (g[:, :, 5] == 0).all()                           # NaN in one field alone: in no bin at all
    # tasmin == tasmax: the day counts of the bins kernel
    T, n = T0, 1025
    x = (np.round(rng.uniform(-4.0, 42.0, (T, n)) * 4) / 4).astype(dtype)
    x[4, 7] = np.nan
    edges = [-INF] + [float(v) for v in np.arange(-2.0, 41.0, 2.75)] + [INF]
    assert all(float(dtype(e)) == e for e in edges)
    win, m01 = _windows(n)
    X = dev(x)
    for kw in ({}, {"doy": DOY, "windows": win}):
        got, st = engine.exposure_reduce(X, X, RB, ROWS, 0.0, edges, **kw)
        cnt, _ = engine.bin_days_reduce(X, RB, ROWS, 0.0, edges, **kw)
        assert int(st.item()) == 0 and torch.equal(got, cnt)
    # +-inf out of season: not a bit, not the status word; in season: bit 0
    lo, hi = _kelvin_pair(5, T, n, dtype)
    kw = {"doy": DOY, "windows": win}
    clean, st = engine.exposure_reduce(dev(lo), dev(hi), RB, ROWS, KELVIN, _edges(17), **kw)
    assert int(st.item()) == 0
    plo, phi = lo.copy(), hi.copy()
    plo[m01 == 0], phi[m01 == 0] = -np.inf, np.inf
    assert (m01 == 0).any()
    got, st = engine.exposure_reduce(dev(plo), dev(phi), RB, ROWS, KELVIN, _edges(17), **kw)
    assert int(st.item()) == 0 and torch.equal(got, clean)
    t, j = [int(v[0]) for v in np.nonzero((m01 == 1) & np.isin(np.arange(T), ROWS)[:, None])]
    for which, v in ((phi, np.inf), (plo, -np.inf)):
        keep = which[t, j]
        which[t, j] = v
        got, st = engine.exposure_reduce(dev(plo), dev(phi), RB, ROWS, KELVIN, _edges(17), **kw)
        assert int(st.item()) == 1 and bool(torch.isfinite(got).all())
        which[t, j] = keep
    _, st = engine.exposure_reduce(dev(plo), dev(phi), RB, ROWS, KELVIN, _edges(17))      # no season: every inf counts
    assert int(st.item()) == 1


@PADS
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tangency_probes(torch_cuda, dtype, wide):
    """tasmax 1, 2, 4, 16 and 256 ulps above the edge, and tasmin as many below it, each on the first day of a period with nine
    ordinary days: the probe day alone gives finite values in [0, 1] within the bound (D = 1), the period stays within it -- on
    both kernels (row stride 11 / 12)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    dev = lambda host: _dev(torch, host, _pad_for(host.shape[1], wide))       # rows padded to the kernel asked for
    ulps, e, T = (1, 2, 4, 16, 256), 25.0, 10
    rng = np.random.default_rng(9)
    lo = rng.uniform(8.0, 22.0, (T, 2 * len(ulps))).astype(dtype)
    hi = (lo + rng.uniform(2.0, 14.0, lo.shape).astype(dtype)).astype(dtype)
    for i, k in enumerate(ulps):
        up, down = dtype(e), dtype(e)
        for _ in range(k):
            up, down = np.nextafter(up, dtype(np.inf)), np.nextafter(down, dtype(-np.inf))
        lo[0, i], hi[0, i] = dtype(e - 7.0), up                                          # the curve just reaches over the edge
        lo[0, len(ulps) + i], hi[0, len(ulps) + i] = down, dtype(e + 9.0)               # ... just dips under it
    edges = [-INF, e, INF]
    Xlo, Xhi = dev(lo), dev(hi)
    for rb, rows, name in ((np.array([0, 1]), np.array([0]), "the probe day"), (np.array([0, T]), np.arange(T), "its period")):
        D = ER.counted_days(lo, hi, rb, rows)
        want = ER.exposure_bins(lo, hi, 0.0, edges, rb, rows)
        got, st = engine.exposure_reduce(Xlo, Xhi, rb, rows, 0.0, edges)
        g, ratio = _check(got, want, D, TOL[dtype], name)
        assert int(st.item()) == 0
        if len(rows) == 1:
            assert ((g >= 0) & (g <= 1)).all() and (want[1, 0, :len(ulps)] > 0).all() and (want[0, 0, len(ulps):] > 0).all()
        print("tangency probes %s, %s: ratio to the bound %.3g (above the edge on the probe day: got %r, want %r)" % (
            np.dtype(dtype).name, name, ratio, g[1, 0, :len(ulps)].tolist(), want[1, 0, :len(ulps)].tolist()))


@PADS
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_band_skipping_changes_no_bit(torch_cuda, dtype, wide):
    """A column computed alone (n = 1, no workspace) and inside a 1025-wide field whose other cells put every finite edge inside
    their range on every row (the wave evaluates the arccosine for every edge), and inside one whose other cells keep every edge
    out of band (the wave skips wherever the column itself allows): the same bits, whether the wide field runs the cell-by-cell
    kernel (stride 1025) or the 16-byte one (stride 1028; the column alone is always cell by cell)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    dev = lambda host: _dev(torch, host, _pad_for(host.shape[1], wide))       # rows padded to the kernel asked for
    n, j = 1025, 517
    lo1, hi1 = _kelvin_pair(21, T0, 1, dtype)
    lo1[1, 0] = lo1[5, 0]                                                                # (keep the column's days counted)
    edges = _edges(17)
    alone, st = engine.exposure_reduce(_dev(torch, lo1), _dev(torch, hi1), RB, ROWS, KELVIN, edges, workspace=False)
    assert int(st.item()) == 0 and float(alone.abs().sum()) > 0
    for name, a, b in (("in band", -50.0, 90.0), ("out of band", -60.0, -60.0)):
        lo = np.full((T0, n), 273.15 + a, dtype=dtype)
        hi = np.full((T0, n), 273.15 + b, dtype=dtype)
        lo[:, j], hi[:, j] = lo1[:, 0], hi1[:, 0]
        inside, st = engine.exposure_reduce(dev(lo), dev(hi), RB, ROWS, KELVIN, edges, workspace=False)
        assert int(st.item()) == 0 and torch.equal(inside[:, :, j], alone[:, :, 0]), name


@PADS
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_agreement_with_the_ladder_kernel(torch_cuda, dtype, wide):
    """A = -d EDD / de falls with e, so for thresholds a < b:  (b - a) S(b) <= EDD(a) - EDD(b) <= (b - a) S(a),  S(e) the summed
    bins above e (closing edge +inf), EDD from engine.edd_ladder_reduce on the same fields, lists and season; slack
    tol * (|EDD(a)| + |EDD(b)| + (b - a) D).  n = 255 at row stride 255 (cell by cell) and 256 (16-byte pieces)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    dev = lambda host: _dev(torch, host, _pad_for(host.shape[1], wide))       # rows padded to the kernel asked for
    n, tol = 255, TOL[dtype]
    lo, hi = _kelvin_pair(33, T0, n, dtype)
    win, m01 = _windows(n)
    thr = [float(v) for v in np.linspace(-4.0, 44.0, 25)]
    Xlo, Xhi = dev(lo), dev(hi)
    for kw, m in (({"doy": DOY, "windows": win}, m01), ({}, np.ones_like(m01))):
        D = ER.counted_days(lo, hi, RB, ROWS, m)
        edd, st = engine.edd_ladder_reduce(Xlo, Xhi, RB, ROWS, KELVIN, thr, **kw)
        bins, st2 = engine.exposure_reduce(Xlo, Xhi, RB, ROWS, KELVIN, thr + [INF], **kw)
        assert int(st.item()) == 0 and int(st2.item()) == 0
        edd, bins = edd.double().cpu().numpy(), bins.double().cpu().numpy()
        S = np.cumsum(bins[::-1], axis=0)[::-1]                                          # S[k] = the days above thr[k]
        for k in range(len(thr) - 1):
            w = thr[k + 1] - thr[k]
            diff = edd[k] - edd[k + 1]
            slack = tol * (np.abs(edd[k]) + np.abs(edd[k + 1]) + w * D)
            assert (w * S[k + 1] - slack <= diff).all() and (diff <= w * S[k] + slack).all(), (k, bool(kw))


def _celsius(ds):
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius
    for k in ("tasmin", "tasmax"):
        ds[k].attrs["units"] = "K"
        ds = convert_kelvin_to_celsius(ds, k)
    return ds


def _aggregated(c, lo, hi, edges, mask, rb, rows):
    """the restatement aggregated in NumPy: ((n_bins, P, R) bins, (P, R) aggregated day counts)"""
    from oracle import ref_numpy as O
    G = c.G
    m = np.nan_to_num(mask, nan=0.0)
    daily = ER.day_bins(lo.reshape(c.T, G), hi.reshape(c.T, G), KELVIN, edges) * m[None]
    ok = (~(np.isnan(lo) | np.isnan(hi))).reshape(c.T, G) * m
    agg = lambda f: _psum(O.agg_coded(f, c.cell, c.code, c.w_eff, c.R), rb, rows)
    return np.stack([agg(d) for d in daily]), agg(ok.astype(np.float64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_public_call(torch_cuda, plan_kind, dtype):
    """snyder_exposure_aggregate of Kelvin fields shifted by convert_kelvin_to_celsius, period="year" over a year end and a label
    per day, with and without a season: dims, the bin coordinate, units and bin_edges; every value within tol of the restatement
    aggregated in NumPy, relative to the aggregated day count; cells="referenced" against cells="all" (difference printed);
    results_on_device(); a counted +-inf raises ValueError, tasmin > tasmax what snyder_edd raises."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import periods
    from climate_toolbox_amd.transformations import snyder_exposure_aggregate
    torch = torch_cuda
    T, R, tol = 9, 5, TOL[dtype]
    c = _Case(7, 9, T, R, dtype, seed=41)
    c.time = np.datetime64("2003-12-27") + np.arange(T)
    c.tas[2, 1, 3] = np.nan
    gd, z1, z2 = _seasons_for(c, seed=T)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time))
    edges = [-INF, -8.0, 0.0, 6.5, 12.0, 19.25, 27.0, INF]
    dataset = lambda device=True: _celsius(c.dataset(torch, device=device, tasmin=c.tas, tasmax=c.tasmax))
    call = lambda ds=None, **kw: snyder_exposure_aggregate(ds if ds is not None else dataset(), edges, "popwt", "reg", c.df, **kw)
    worst = 0.0
    for period in ("year", np.arange(T) % 3):
        labels, rb, rows = periods.period_rows(c.time, period)
        for season, m in ((None, np.ones((T, c.G))), (sw, mask)):
            out = call(period=period, season=season)
            v = out["exposure"]
            assert v.dims == ("bin", "period", "reg") and v.attrs["units"] == "days"
            assert v.attrs["bin_edges"] == ", ".join(repr(float(e)) for e in edges)
            assert out["bin"].values.dtype == np.float64 and list(out["bin"].values) == edges[:-1]
            np.testing.assert_array_equal(out["period"].values, labels)
            got = v.values
            assert isinstance(v.data, np.ndarray) and got.dtype == dtype and got.shape == (len(edges) - 1, len(labels), R)
            assert np.isnan(got[:, :, R - 1]).all()                                      # the region without weight
            want, Dagg = _aggregated(c, c.tas, c.tasmax, edges, m, rb, rows)
            err = np.abs(got[:, :, :R - 1] - want[:, :, :R - 1])
            bound = tol * Dagg[None, :, :R - 1]
            assert (err <= bound).all(), (period, season is not None, float(err.max()))
            full = np.broadcast_to(bound, err.shape)
            worst = max(worst, float(np.max(err[full > 0] / full[full > 0])))
            ref = call(period=period, season=season, cells="referenced")["exposure"].values
            diff = np.abs(ref[:, :, :R - 1] - got[:, :, :R - 1])
            print("public call %s, %s: cells='referenced' vs 'all', largest difference %.3g days" % (np.dtype(dtype).name, plan_kind, diff.max()))
            assert (diff <= 2 * bound).all()                                             # (each within tol of the same restatement)
    print("public call %s, %s: largest ratio to the bound %.3g" % (np.dtype(dtype).name, plan_kind, worst))
    seasonal = call(period="year", season=sw)["exposure"].values
    np.testing.assert_array_equal(call(dataset(device=False), period="year", season=sw)["exposure"].values, seasonal)
    other = call(period="year", season=sw, varname="hours", tasmin="tasmin", tasmax="tasmax")
    np.testing.assert_array_equal(other["hours"].values, seasonal)
    with pkg.results_on_device():
        on = call(period="year", season=sw)
        assert isinstance(on["exposure"].data, torch.Tensor) and on["exposure"].data.is_cuda
        assert tuple(on["exposure"].data.shape) == seasonal.shape
    np.testing.assert_array_equal(on["exposure"].values, seasonal)
    # a counted +-inf raises; out of season it is nobody's business
    m3 = mask.reshape(T, c.nlat, c.nlon)
    t, i, j = [int(x[0]) for x in np.nonzero(m3 == 0)]
    keep = c.tasmax[t, i, j]
    c.tasmax[t, i, j] = np.inf
    np.testing.assert_array_equal(call(period="year", season=sw)["exposure"].values, seasonal)
    with pytest.raises(ValueError, match="inf"):
        call(period="year")
    c.tasmax[t, i, j] = keep
    t, i, j = [int(x[0]) for x in np.nonzero(m3 == 1)]
    keep = c.tasmax[t, i, j]
    c.tasmax[t, i, j] = np.inf
    with pytest.raises(ValueError, match="inf"):
        call(period="year", season=sw)
    c.tasmax[t, i, j] = c.tas[t, i, j] - dtype(1.0)                                      # tasmin > tasmax: snyder_edd's own refusal
    with pytest.raises(AssertionError, match="tasmin > tasmax"):
        call(period="year", season=sw)
    c.tasmax[t, i, j] = keep


def test_seventy_bins_run_in_two_launches(torch_cuda, plan_kind, monkeypatch):
    """71 edges through seasons._exposure_totals: 64 bins, then 6, the launches sharing edge 64 -- and the whole equals ONE
    restatement with all 71 edges."""
    from climate_toolbox_amd import engine, periods
    from climate_toolbox_amd.transformations import snyder_exposure_aggregate
    torch = torch_cuda
    dtype = np.float64
    c = _Case(7, 9, 9, 5, dtype, seed=23)
    edges = [-INF] + [float(v) for v in np.linspace(-30.0, 45.0, 69)] + [INF]
    ran = []
    real = engine.exposure_reduce
    monkeypatch.setattr(engine, "exposure_reduce", lambda *a, **k: (ran.append(len(a[5])), real(*a, **k))[1])
    ds = _celsius(c.dataset(torch, tasmin=c.tas, tasmax=c.tasmax))
    out = snyder_exposure_aggregate(ds, edges, "popwt", "reg", c.df, period="month")
    assert ran == [65, 7]
    v = out["exposure"].values
    assert v.shape == (70, 1, c.R) and list(out["bin"].values) == edges[:-1]
    labels, rb, rows = periods.period_rows(c.time, "month")
    want, Dagg = _aggregated(c, c.tas, c.tasmax, edges, np.ones((c.T, c.G)), rb, rows)
    assert (np.abs(v[:, :, :c.R - 1] - want[:, :, :c.R - 1]) <= TOL[dtype] * Dagg[None, :, :c.R - 1]).all()
    np.testing.assert_allclose(v[:, :, :c.R - 1].sum(0), c.T, rtol=1e-6)                 # every day is somewhere in the 70 bins
