"""Temperature-bin day counts on the GPU (run with -m gpu): wagg_bin_days_reduce_* through engine.bin_days_reduce against a NumPy
restatement, and tas_bins_aggregate on both plan kinds against the period call on one 0/1 field per bin -- at the shapes,
windows and period structures of tests/test_gpu_periods.py and tests/test_gpu_seasons.py.

The restatement: c = edges - offset in fp64; a day counts for bin k iff float64(x) >= c[k] and float64(x) < c[k + 1] and the
cell is in season; summed over each period's row list.  Counts are compared EXACTLY, never by tolerance."""
import os

import numpy as np
import pytest

from tests.test_gpu_packed_totals import _Sparse, _rel, segment_plans  # noqa: F401
from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok  # noqa: F401
from tests.test_gpu_periods import CASES, _Case, _field, _psum, _structures
from tests.test_gpu_seasons import KELVIN, _doys, _mask_TG, _mixed_cells, _pack, _seasons_for, plan_kind  # noqa: F401
from tests.test_seasons_host import ref_mask

pytestmark = pytest.mark.gpu

INF = float("inf")
A_EQ, A_ULP, A_NINF, A_PINF = 12, 18, 24, 30    # open-all-year cells (j % 6 == 0) that carry the special values


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _restate(X, m01, rb, rows, edges, offset):
    """(n_bins, P, n) day counts in fp64: the module docstring's rule"""
    x64 = np.asarray(X, dtype=np.float64)
    c = np.asarray(edges, dtype=np.float64) - np.float64(offset)
    with np.errstate(invalid="ignore"):
        return np.stack([_psum((x64 >= c[k]) & (x64 < c[k + 1]) & (m01 > 0), rb, rows) for k in range(len(c) - 1)])


def _exact(got, want, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%r: %d counts differ, first at (bin, period, cell) %r: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,pad", [(63, 0), (63, 3), (1100, 3)])
@pytest.mark.parametrize("T", [9, 70])
def test_counts_equal_the_restatement(torch_cuda, dtype, n, pad, T):
    """A Kelvin field with offset -273.15 and 64 bins in degrees C (-inf first, +inf last), under mixed windows (null, empty,
    single-day, wrapping, open) and without a season, for every period structure (T = 70 with one period: the split path;
    "interleaved": an empty period); aligned rows whose last piece is partial, rows that are not 16-byte aligned (pad = 3: the
    cell-by-cell kernel) and more than one column block.  Among the edges: one equal to a cell's own value + offset (that
    cell lands in the upper bin) and one an ulp of the element type above a cell's value (that cell lands in the lower bin).
    Shorter lists of 2, 3, G + 1, G + 2 and 17 edges, with and without infinite ends, equal the restatement and the matching
    planes (or, for an open end bin, the sum of the planes it covers) of the longest; two runs are bit-equal; with both ends
    open the bins sum to the in-season days whose value is neither NaN nor +inf.  A NaN in season and a NaN cell count
    nowhere with status 0; NaN, +inf and 1e30 out of season change no count and no status; an in-season -inf lands in the open
    first bin, an in-season +inf in none, and either sets bit 0.  Without the workspace (no split) the counts are the same."""
    from climate_toolbox_amd import _lib, engine
    from climate_toolbox_amd.periods import period_rows
    torch = torch_cuda
    G = _lib.BIN_GROUP
    rng = np.random.default_rng(100 * T + n + pad)
    _, X = _field(rng, T, n, pad, dtype, torch)
    tdt = torch.float32 if dtype == np.float32 else torch.float64

    def strided(host):
        buf = torch.zeros((T, n + pad), dtype=tdt, device="cuda")
        buf[:, :n] = torch.from_numpy(host).cuda()
        return buf[:, :n]

    X[0, 0] = np.nan                                    # (cell 0 is open all year: NaN in season)
    X[:, 6] = np.nan                                    # NaN on every day, in a cell that is open all year
    X[0, A_EQ], X[0, A_ULP] = dtype(291.3125), dtype(284.7)
    Xd = strided(X)
    assert Xd.stride(0) == n + pad
    # the edges, in degrees C: 61 across the data, the two special ones, open ends
    e_eq = float(X[0, A_EQ]) + KELVIN                   # c = e_eq - KELVIN is the cell's value itself ...
    up = np.nextafter(X[0, A_ULP], dtype(np.inf))
    e_ulp = float(up) + KELVIN                          # ... and here the next value of the element type above the cell's
    assert e_eq - KELVIN == float(X[0, A_EQ]) and e_ulp - KELVIN == float(up) and float(up) > float(X[0, A_ULP])
    inner = np.sort(np.concatenate([np.linspace(-38.0, 51.0, 61), [e_eq, e_ulp]]))
    full = np.concatenate([[-INF], inner, [INF]])
    assert len(full) == 65 == _lib.BIN_EDGES_MAX and (np.diff(full) > 0).all()
    k_eq, k_ulp = int(np.flatnonzero(full == e_eq)[0]), int(np.flatnonzero(full == e_ulp)[0])
    sizes = sorted({2, 3, G + 1, G + 2, 17})
    assert len(sizes) == 5
    dead = torch.from_numpy(np.flatnonzero((np.arange(n) % 6 == 1) | (np.arange(n) % 6 == 2))).cuda()
    for si, (name, lab) in enumerate(_structures(T)):
        labels, rb, rows = period_rows(np.arange(T), lab)
        if name == "interleaved":                       # ... with an empty period in the middle
            rb = np.concatenate([rb[:1], rb[:1], rb[1:]])
        P = len(rb) - 1
        dname, doy = _doys(T)[si % 3]
        z1, z2 = _mixed_cells(n, doy)
        win = _pack(z1, z2)
        m01 = np.nan_to_num(ref_mask(z1, z2, doy), nan=0.0).T                     # (T, n)
        for season, m in ((True, m01), (False, np.ones_like(m01))):
            kw = {"doy": doy, "windows": win} if season else {}
            what = (name, dname if season else "no season")
            got, st = engine.bin_days_reduce(Xd, rb, rows, KELVIN, full, **kw)
            assert got.shape == (64, P, n) and got.dtype == tdt and int(st.item()) == 0, what
            want = _restate(X, m, rb, rows, full, KELVIN)
            _exact(got, want, what)
            again, _ = engine.bin_days_reduce(Xd, rb, rows, KELVIN, full, **kw)
            assert torch.equal(again, got), what                                  # bit-reproducible
            whole, _ = engine.bin_days_reduce(Xd, rb, rows, KELVIN, full, workspace=False, **kw)
            assert torch.equal(whole, got), what                                  # every split gives the same counts
            # both ends open: the bins sum to the days that count at all
            with np.errstate(invalid="ignore"):
                days = _psum((m > 0) & ~np.isnan(X) & (X != np.inf), rb, rows)
            assert np.array_equal(got.double().sum(0).cpu().numpy(), days), what
            assert (got[:, :, 6] == 0).all(), what                                # the NaN cell is in no bin
            if season:
                assert (got[:, :, dead] == 0).all(), what                         # null and empty windows: 0 in all 64 bins
            if name == "interleaved":
                assert (got[:, 0] == 0).all(), what                               # the empty period totals 0
            p0 = int(np.flatnonzero([0 in rows[rb[p]:rb[p + 1]] for p in range(P)])[0])      # the period that lists row 0
            on_row0 = lambda j: _restate(X[:1], m[:1], [0, 1], [0], full, KELVIN)[:, 0, j]
            assert on_row0(A_EQ)[k_eq] == 1 and on_row0(A_EQ)[k_eq - 1] == 0      # value == edge: the upper bin
            assert on_row0(A_ULP)[k_ulp - 1] == 1 and on_row0(A_ULP)[k_ulp] == 0  # edge one ulp above the value: the lower bin
            assert float(got[k_eq, p0, A_EQ]) >= 1 and float(got[k_ulp - 1, p0, A_ULP]) >= 1
            # shorter lists: other groups, a ragged last one; closed ends and open ends
            for mlen in sizes:
                a = 1 + (7 * mlen) % (64 - mlen)                                  # an interior slice full[a : a + mlen]
                closed = full[a:a + mlen]
                part, st = engine.bin_days_reduce(Xd, rb, rows, KELVIN, closed, **kw)
                assert part.shape == (mlen - 1, P, n) and int(st.item()) == 0
                assert torch.equal(part, got[a:a + mlen - 1]), (what, mlen, "closed")
                _exact(part, _restate(X, m, rb, rows, closed, KELVIN), (what, mlen, "closed"))
                opened = np.concatenate([[-INF], closed[1:-1], [INF]])
                part, st = engine.bin_days_reduce(Xd, rb, rows, KELVIN, opened, **kw)
                assert part.shape == (mlen - 1, P, n) and int(st.item()) == 0
                _exact(part, _restate(X, m, rb, rows, opened, KELVIN), (what, mlen, "open"))
                if mlen == 2:
                    assert torch.equal(part[0], got.sum(0)), (what, "one bin")
                else:
                    assert torch.equal(part[1:-1], got[a + 1:a + mlen - 2]), (what, mlen, "open")
                    assert torch.equal(part[0], got[:a + 1].sum(0)) and torch.equal(part[-1], got[a + mlen - 2:].sum(0)), (what, mlen, "ends")
            if not season:
                continue
            # whatever stands out of season is never looked at
            Xp = X.copy()
            poison = np.array([np.nan, np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 3]
            Xp[m01 == 0] = poison[m01 == 0]
            g2, st = engine.bin_days_reduce(strided(Xp), rb, rows, KELVIN, full, **kw)
            assert torch.equal(g2, got) and int(st.item()) == 0, what
    # row 0 alone, no season: the cell on the edge is in the upper bin, the cell one ulp below its edge in the lower one
    one, _ = engine.bin_days_reduce(Xd, [0, 1], [0], KELVIN, full)
    assert float(one[k_eq, 0, A_EQ]) == 1 and float(one[k_eq - 1, 0, A_EQ]) == 0
    assert float(one[k_ulp - 1, 0, A_ULP]) == 1 and float(one[k_ulp, 0, A_ULP]) == 0
    # in-season infinities (cells A_NINF and A_PINF are open all year; rows 1 and 2 are listed): -inf in the open first bin and,
    # under a closed first edge, in none; +inf in no bin; bit 0 either way, with and without a season
    doy = _doys(T)[0][1]
    z1, z2 = _mixed_cells(n, doy)
    win = _pack(z1, z2)
    m01 = np.nan_to_num(ref_mask(z1, z2, doy), nan=0.0).T
    rb, rows = np.array([0, T]), np.arange(T)
    for j, v, t in ((A_NINF, -np.inf, 1), (A_PINF, np.inf, 2)):
        Xi = X.copy()
        Xi[t, j] = v
        for kw, m in (({"doy": doy, "windows": win}, m01), ({}, np.ones_like(m01))):
            got, st = engine.bin_days_reduce(strided(Xi), rb, rows, KELVIN, full, **kw)
            assert int(st.item()) == 1
            _exact(got, _restate(Xi, m, rb, rows, full, KELVIN), ("inf", v))
            in_bins = got[:, 0, j].double().sum().item()
            assert in_bins == (T if v < 0 else T - 1) and float(got[0, 0, j]) >= (1 if v < 0 else 0)
            closed, st = engine.bin_days_reduce(strided(Xi), rb, rows, KELVIN, full[1:-1], **kw)
            assert int(st.item()) == 1 and torch.equal(closed, got[1:-1])
            _exact(closed, _restate(Xi, m, rb, rows, full[1:-1], KELVIN), ("inf, closed ends", v))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fields_in_their_own_units_and_the_binding(torch_cuda, dtype):
    """offset 0: the edges are in the field's units; an edge equal to a value takes it into the upper bin, an edge one ulp above
    leaves it in the lower one -- in fp32 too, where the fp64 edge 0.1 is no float: float32(0.1) > 0.1 lies in [0.1, ...), its
    predecessor below.  The binding refuses what the library would."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    T, n = 9, 63
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    v = dtype(0.1)
    X = np.full((T, n), 2.0, dtype=dtype)
    X[0, 5], X[1, 5], X[2, 5], X[3, 5] = v, np.nextafter(v, dtype(-1)), np.nextafter(v, dtype(1)), dtype(-0.0)
    Xd = torch.from_numpy(X).cuda()
    rb, rows = [0, T], np.arange(T)
    for edges in ([0.0, 0.1, float(v), float(np.nextafter(v, dtype(1))), 2.0, 2.5], [-1.0, 0.1, 3.0], [float(v), 3.0]):
        if len(set(edges)) != len(edges):
            edges = sorted(set(edges))
        got, st = engine.bin_days_reduce(Xd, rb, rows, 0.0, edges)
        assert got.dtype == tdt and int(st.item()) == 0
        _exact(got, _restate(X, np.ones((T, n)), np.asarray(rb), rows, edges, 0.0), edges)
    got, _ = engine.bin_days_reduce(Xd, rb, rows, 0.0, [-1.0, 0.1, 3.0])
    want_low = 1 + int(float(v) < 0.1) + int(float(np.nextafter(v, dtype(-1))) < 0.1)       # -0.0, and what lies below the fp64 0.1
    assert float(got[0, 0, 5]) == want_low and float(got[1, 0, 5]) == T - want_low and float(got[1, 0, 7]) == T
    with pytest.raises(ValueError, match="edges"):
        engine.bin_days_reduce(Xd, rb, rows, 0.0, list(range(_lib.BIN_EDGES_MAX + 1)))
    with pytest.raises(ValueError, match="edges"):
        engine.bin_days_reduce(Xd, rb, rows, 0.0, [1.0])
    with pytest.raises(ValueError, match="ascend"):
        engine.bin_days_reduce(Xd, rb, rows, 0.0, [1.0, 1.0])
    with pytest.raises(ValueError, match="ascend"):
        engine.bin_days_reduce(Xd, rb, rows, 0.0, [0.0, float("nan")])
    with pytest.raises(ValueError, match="go together"):
        engine.bin_days_reduce(Xd, rb, rows, 0.0, [0.0, 1.0], doy=np.arange(1, T + 1))
    with pytest.raises(ValueError):
        engine.bin_days_reduce(Xd, rb, rows, 0.0, [0.0, 1.0], doy=np.arange(1, T), windows=np.zeros(n, dtype=np.int32))


EDGES = [-INF, -12.0, 0.0, 5.5, 11.0, 19.25, 30.0, INF]


def _zero_one(c, k, edges, offset):
    """the 0/1 field of bin k, made the restatement's way, in the case's element type"""
    x64 = c.tas.astype(np.float64)
    cc = np.asarray(edges, dtype=np.float64) - np.float64(offset)
    return ((x64 >= cc[k]) & (x64 < cc[k + 1])).astype(c.dtype)


@pytest.mark.parametrize("nlat,nlon,T,R,dtype", CASES)
def test_public_call_on_both_plan_kinds(torch_cuda, plan_kind, tmp_path, nlat, nlon, T, R, dtype):
    """tas_bins_aggregate of a Kelvin-shifted field with period="year" and "month" (the days run over a year end), with and
    without a season: every bin plane against weighted_aggregate_grid_to_regions_periods of that bin's 0/1 field -- the way of
    the commit before -- at the tolerances of tests/test_gpu_parity.py (the contraction is the same code); dims, the bin
    coordinate and the attributes; a plain field with the edges in kelvin gives the same numbers; (lat, lon, time) and
    host-resident fields give the same numbers; results_on_device(); leap_days="drop"; a netCDF round trip."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import minixr
    from climate_toolbox_amd.output import read_netcdf, to_netcdf
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, remove_leap_days, tas_bins_aggregate
    torch = torch_cuda
    c = _Case(nlat, nlon, T, R, dtype, seed=nlat + T + R)
    c.time = np.datetime64("2003-12-27") + np.arange(T)                           # 5 days of 2003, the rest of 2004 (29 February in T = 70)
    c.tas[0, 0, 1] = dtype(283.15)                                                # a value on the edge 10.0 - (-273.15) ...
    edges = EDGES[:4] + [float(np.float64(c.tas[0, 0, 1]) + KELVIN)] + EDGES[4:]  # ... whatever fp64 makes of that sum
    gd, z1, z2 = _seasons_for(c, seed=T)
    sw = pkg.season_windows(gd)
    nb = len(edges) - 1

    def dataset(device=True, moved=False, kelvin=True):
        if not moved:
            ds = c.dataset(torch, device=device)
        else:
            wrap = (lambda v: torch.from_numpy(v).cuda()) if device else (lambda v: v)
            ds = minixr.Dataset({"tas": (("lat", "lon", "time"), wrap(np.ascontiguousarray(np.moveaxis(c.tas, 0, -1))))},
                                coords={"time": c.time, "lat": c.lat, "lon": c.lon})
        return convert_kelvin_to_celsius(ds, "tas") if kelvin else ds

    call = lambda ds, e=edges, **kw: tas_bins_aggregate(ds, e, "popwt", "reg", c.df, **kw)
    first = None
    for period in ("year", "month"):
        for season in (None, sw):
            out = call(dataset(), period=period, season=season)
            v = out["tas-bins"]
            assert v.dims == ("bin", "period", "reg") and v.attrs["units"] == "days"
            assert v.attrs["bin_edges"] == ", ".join(repr(float(e)) for e in edges)
            assert out["bin"].values.dtype == np.float64 and list(out["bin"].values) == edges[:-1]
            got = v.values
            assert isinstance(v.data, np.ndarray) and got.dtype == dtype and got.shape[0] == nb and got.shape[2] == R
            assert np.isnan(got[:, :, R - 1]).all()                               # the region without weight
            for k in range(nb):
                ds01 = c.dataset(torch, tas=_zero_one(c, k, edges, KELVIN))
                ref = pkg.weighted_aggregate_grid_to_regions_periods(ds01, "tas", "popwt", "reg", c.df, period=period, season=season)
                np.testing.assert_array_equal(out["period"].values, ref["period"].values)
                _rel_ok(got[k], ref["tas"].values, c.rtol)
            if first is None:
                first = got
            if period == "year" and season is sw:
                seasonal = got
    assert T == 1 or first.shape[1] == 2
    kw = dict(period="year", season=sw)
    # a plain field, the edges in kelvin: c = edge - 0 must be the same fp64 numbers for the counts to be the same
    k_edges = [e - KELVIN for e in edges]                                         # (the library forms the same difference)
    np.testing.assert_array_equal(call(dataset(kelvin=False), k_edges, **kw)["tas-bins"].values, seasonal)
    # other layouts and residencies: the same kernels on the same numbers
    np.testing.assert_array_equal(call(dataset(device=False), **kw)["tas-bins"].values, seasonal)
    moved = call(dataset(moved=True), **kw)
    assert moved["tas-bins"].dims == ("bin", "reg", "period")
    np.testing.assert_array_equal(np.swapaxes(moved["tas-bins"].values, 1, 2), seasonal)
    np.testing.assert_array_equal(np.swapaxes(call(dataset(device=False, moved=True), **kw)["tas-bins"].values, 1, 2), seasonal)
    other = call(dataset(), varname="days", tas="tas", **kw)
    np.testing.assert_array_equal(other["days"].values, seasonal)
    with pkg.results_on_device():
        on = call(dataset(), **kw)
        assert isinstance(on["tas-bins"].data, torch.Tensor) and on["tas-bins"].data.is_cuda
        assert tuple(on["tas-bins"].data.shape) == seasonal.shape
        assert isinstance(call(dataset(device=False), **kw)["tas-bins"].data, np.ndarray)     # (a host-resident field's: a host array)
    np.testing.assert_array_equal(on["tas-bins"].values, seasonal)
    # leap days: "drop" is remove_leap_days first; "keep" counts 29 February like any day
    dropped = call(dataset(), period="year", leap_days="drop")["tas-bins"].values
    np.testing.assert_array_equal(dropped, call(remove_leap_days(dataset()), period="year")["tas-bins"].values)
    kept = call(dataset(), period="year")["tas-bins"].values
    has_leap = bool((c.time == np.datetime64("2004-02-29")).any())
    assert has_leap == (T == 70) and np.array_equal(dropped, kept, equal_nan=True) != has_leap
    # the file: values and attributes survive
    path = os.path.join(str(tmp_path), "bins.nc")
    to_netcdf(call(dataset(), **kw), path)
    back = read_netcdf(path)
    np.testing.assert_array_equal(back["tas-bins"].values, seasonal)
    assert back["tas-bins"].attrs["bin_edges"] == ", ".join(repr(float(e)) for e in edges) and back["tas-bins"].attrs["units"] == "days"
    np.testing.assert_array_equal(back["bin"].values, np.asarray(edges[:-1]))


def test_in_season_inf_raises(torch_cuda, plan_kind):
    """+-inf out of season is nobody's business; counted, it raises ValueError -- with and without a season."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd.transformations import tas_bins_aggregate
    torch = torch_cuda
    c = _Case(7, 9, 9, 5, np.float64, seed=3)
    gd, z1, z2 = _seasons_for(c, seed=8)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time)).reshape(c.T, c.nlat, c.nlon)
    edges = [e - KELVIN for e in EDGES]                                           # (the field stays in kelvin: a plain field)
    call = lambda season=sw: tas_bins_aggregate(c.dataset(torch), edges, "popwt", "reg", c.df, period="year", season=season)["tas-bins"].values
    clean = call()
    t, i, j = [int(v[0]) for v in np.nonzero(mask == 0)]
    keep = c.tas[t, i, j]
    c.tas[t, i, j] = np.inf
    np.testing.assert_array_equal(call(), clean)
    with pytest.raises(ValueError, match="inf"):
        call(None)
    c.tas[t, i, j] = keep
    t, i, j = [int(v[0]) for v in np.nonzero(mask == 1)]
    c.tas[t, i, j] = -np.inf
    with pytest.raises(ValueError, match="inf"):
        call()
    c.tas[t, i, j] = np.nan                                                       # NaN is in no bin and raises nothing
    assert np.isfinite(call()[:, :, :c.R - 1]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_referenced_cells(torch_cuda, segment_plans, dtype):
    """cells="referenced" on a segment-table plan with a quads map: it packs, and equals cells="all" to the rounding of the
    contraction (the counts themselves are the same integers; the two contractions add them in different orders) -- the
    largest relative difference is printed; with and without a season, device- and host-resident; a +inf in a quad no row
    reads does not raise, where cells="all" does."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_bins_aggregate
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=19)
    c.time = np.datetime64("2003-12-12") + np.arange(c.T)
    gd, z1, z2 = _seasons_for(c, seed=c.T)
    sw = pkg.season_windows(gd)
    packs = lambda: engine.PACK_STATS["device"] + engine.PACK_STATS["host"] + engine.PACK_STATS["host_fallback"]
    in_row = c.plan().compact_cells(dtype)
    assert in_row is not None
    ds = lambda device=True, f=c.tas: convert_kelvin_to_celsius(c.dataset(torch, device=device, tas=f), "tas")
    for season in (sw, None):
        call = lambda cells, d=None: tas_bins_aggregate(d or ds(), EDGES, "popwt", "reg", c.df, period="year", season=season,
                                                        cells=cells)["tas-bins"].values
        n0 = packs()
        got = call("referenced")
        assert packs() > n0
        n0 = packs()
        old = call("all")
        assert packs() == n0
        print("16x32 %s, bins%s: referenced vs all, max rel diff %.3g" % (np.dtype(dtype).name, ", season" if season is not None else "",
                                                                          _rel(got, old)))
        assert got.shape == old.shape == (len(EDGES) - 1, 2, c.R)
        _rel_ok(got, old, c.rtol)
        np.testing.assert_array_equal(call("referenced", ds(device=False)), got)
        poisoned = c.poisoned(c.tas, in_row)
        np.testing.assert_array_equal(call("referenced", ds(f=poisoned)), got)   # NaN and +-inf in quads no row reads: nothing
        if season is None:
            with pytest.raises(ValueError, match="inf"):
                call("all", ds(f=poisoned))


def test_referenced_cells_fall_back_on_a_dense_family_plan(torch_cuda, monkeypatch):
    """a dense-family plan has no quads map: cells="referenced" packs nothing and equals cells="all" bit for bit"""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _plans, engine
    from climate_toolbox_amd.transformations import tas_bins_aggregate
    torch = torch_cuda
    pkg.clear_caches()
    monkeypatch.setattr(_plans, "_wants_dense", lambda n_ucells, G, layout, **k: layout == "TG")
    c = _Sparse(16, 32, np.float32, seed=11)
    before = dict(engine.PACK_STATS)
    try:
        edges = [e - KELVIN for e in EDGES]
        call = lambda cells: tas_bins_aggregate(c.dataset(torch), edges, "popwt", "reg", c.df, period="year", cells=cells)["tas-bins"].values
        np.testing.assert_array_equal(call("referenced"), call("all"))
        assert engine.PACK_STATS == before
        assert {type(p).__name__ for p in _plans._PLAN_CACHE.values()} == {"DensePlan"}
    finally:
        pkg.clear_caches()


def test_seventy_bins_run_in_two_launches(torch_cuda, plan_kind, monkeypatch):
    """71 edges: 64 bins, then 6, joined in order -- the two halves called separately, bit for bit"""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_bins_aggregate
    torch = torch_cuda
    c = _Case(7, 9, 9, 5, np.float32, seed=23)
    edges = [-INF] + list(np.linspace(-30.0, 45.0, 69)) + [INF]
    ran = []
    real = engine.bin_days_reduce
    monkeypatch.setattr(engine, "bin_days_reduce", lambda *a, **k: (ran.append(len(a[4])), real(*a, **k))[1])
    call = lambda e: tas_bins_aggregate(convert_kelvin_to_celsius(c.dataset(torch), "tas"), e, "popwt", "reg", c.df, period="month")
    out = call(edges)
    assert ran == [65, 7]
    v = out["tas-bins"].values
    assert v.shape == (70, 1, c.R) and list(out["bin"].values) == edges[:-1]
    np.testing.assert_array_equal(v[:64], call(edges[:65])["tas-bins"].values)
    np.testing.assert_array_equal(v[64:], call(edges[64:])["tas-bins"].values)
    # every day of a region's cells is in exactly one of the 70 bins: the planes sum to the period's days
    np.testing.assert_allclose(v[:, :, :c.R - 1].sum(0), c.T, rtol=1e-4)
