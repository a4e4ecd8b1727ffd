"""Growing-season totals on the GPU (run with -m gpu): wagg_season_reduce_* through engine.season_reduce, wagg_season_mask, and
``season=`` of weighted_aggregate_grid_to_regions_periods / tas_poly_aggregate on both plan kinds, at the smallest shapes at
which the kernel can go wrong (those of tests/test_gpu_periods.py).

Oracle: the reference's mask (utils.py:83-153) restated on plain arrays (tests/test_seasons_host.py: ref_mask) times the daily
field, a plain fp64 sum per period (kernel) or oracle.ref_numpy.agg_coded on the masked daily field and then the sum (public
calls).  Tolerances: the project's own, as tests/test_gpu_periods.py uses them."""
import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok
from tests.test_gpu_periods import SUM_TOL, _Case, _field, _ok, _psum, _structures
from tests.test_seasons_host import ref_mask

pytestmark = pytest.mark.gpu

KELVIN = -273.15
OPEN = 0 | 1023 << 10                                   # a window open all year


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _pack(z1, z2):
    """integer planting / harvest days -> packed windows, by the layout of include/wagg.h (the test's own packing)"""
    out = np.empty(len(z1), dtype=np.int32)
    for j, (p, h) in enumerate(zip(z1, z2)):
        if p != p:
            out[j] = 1 | 1 << 21                                             # null
        elif h != h:
            out[j] = 1 | 1 << 20                                             # no harvest day: the complement of nothing
        elif min(p, h) > 1023 or max(p, h) < 0:
            out[j] = 1 | (1 << 20 if h < p else 0)                           # an empty interval (or its complement)
        else:                                                                # (days clamped to what ten bits hold)
            out[j] = int(max(min(p, h), 0)) | int(min(max(p, h), 1023)) << 10 | (1 << 20 if h < p else 0)
    return out


def _mixed_cells(n, days):
    """(z1, z2) per cell, cycling through: open all year, null, empty, a single day, a plain interval, a wrapping one --
    placed around the days the test's rows carry"""
    lo, hi = int(min(days)), int(max(days))
    z1, z2 = np.empty(n), np.empty(n)
    for j in range(n):
        kind = j % 6
        if kind == 0:
            z1[j], z2[j] = 0, 1023
        elif kind == 1:
            z1[j], z2[j] = np.nan, 150
        elif kind == 2:
            z1[j], z2[j] = 2000, 3000
        elif kind == 3:
            z1[j] = z2[j] = days[(j // 6) % len(days)]
        elif kind == 4:
            z1[j], z2[j] = lo + (j // 6) % 5, lo + 3 + (j // 6) % 41
        else:
            z1[j], z2[j] = hi - (j // 6) % 7, lo + 1 + (j // 6) % 4          # harvest before planting: wraps
    return z1, z2


def _doys(T):
    """day-of-year vectors of T rows: consecutive days, a run across a year end, the same with a day 366"""
    k = T // 2
    return [("consecutive", np.arange(100, 100 + T)),
            ("year end", np.concatenate([np.arange(365 - k + 1, 366), np.arange(1, T - k + 1)])),
            ("leap", np.concatenate([np.arange(366 - k + 1, 367), np.arange(1, T - k + 1)]))]


# ---------------------------------------------------------------------------------------------------------------------
# the kernel, through engine.season_reduce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,rtol", [(np.float32, RTOL32), (np.float64, RTOL64)])
@pytest.mark.parametrize("n,pad", [(63, 0), (63, 3), (256, 0), (1100, 0), (1100, 3)])
@pytest.mark.parametrize("T", [1, 9, 70])
def test_kernel_sums_match_numpy(torch_cuda, dtype, rtol, n, pad, T):
    """Plain sums, four powers and three thresholds under mixed windows, for every period structure of the periods test
    (T = 70 with one period: the split path; "interleaved": an empty period) and three day-of-year vectors; bit-reproducible;
    all-year windows = wagg_period_reduce_* bit for bit; null and empty windows total exactly 0; whatever stands out of season
    -- NaN, +inf, 1e30 -- changes no bit and leaves the status word 0; one in-season +inf sets its bit 0."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.periods import period_rows
    from oracle import ref_numpy as O
    torch = torch_cuda
    rng = np.random.default_rng(100 * T + n + pad)
    Xd, X = _field(rng, T, n, pad, dtype, torch)
    H = (X + rng.uniform(0, 12, X.shape)).astype(dtype)

    def strided(host):
        buf = torch.zeros((T, n + pad), dtype=Xd.dtype, device="cuda")
        buf[:, :n] = torch.from_numpy(host).cuda()
        return buf[:, :n]

    Hd = strided(H)
    assert Xd.stride(0) == n + pad
    X[0, 0] = np.nan                                    # (cell 0 is open all year: NaN in season)
    X[:, 6] = np.nan                                    # NaN on every day, in a cell that is open all year
    Xd.copy_(torch.from_numpy(X).cuda())
    thr = [float(X[0, 1] + dtype(KELVIN)), 12.5, float(H[0, 2] + dtype(KELVIN))]
    open_all = np.full(n, OPEN, dtype=np.int32)
    fpoly = [np.nan_to_num(O.tas_poly_values(X, k + 1), nan=0.0) for k in range(4)]
    fedd = [np.nan_to_num(engine.transform_edd(Xd, Hd, KELVIN, [(1.0, e)]).cpu().numpy(), nan=0.0) for e in thr]
    oedd = [np.nan_to_num(O.snyder_edd_values(X + dtype(KELVIN), H + dtype(KELVIN), e), nan=0.0) for e in thr]
    for si, (name, lab) in enumerate(_structures(T)):
        labels, rb, rows = period_rows(np.arange(T), lab)
        if name == "interleaved":                       # ... with an empty period in the middle
            rb = np.concatenate([rb[:1], rb[:1], rb[1:]])
        P = len(rb) - 1
        for di, (dname, doy) in enumerate(_doys(T)):
            z1, z2 = _mixed_cells(n, doy)
            win = _pack(z1, z2)
            m = ref_mask(z1, z2, doy)                                             # (n, T): 0 / 1 / NaN
            assert np.isnan(m[1]).all() and (m[0] == 1).all() and (m[2] == 0).all()
            m01 = np.nan_to_num(m, nan=0.0).T                                     # (T, n)
            # plain sums
            got, st = engine.season_reduce(Xd, rb, rows, doy, win)
            assert got.shape == (1, P, n) and int(st.item()) == 0
            f = np.nan_to_num(X, nan=0.0)
            _ok(got[0].cpu().numpy(), _psum(m01 * f, rb, rows), SUM_TOL[dtype], _psum(m01 * np.abs(f), rb, rows))
            again, _ = engine.season_reduce(Xd, rb, rows, doy, win)
            assert torch.equal(again, got)                                        # bit-reproducible
            dead = torch.from_numpy(np.flatnonzero((np.arange(n) % 6 == 1) | (np.arange(n) % 6 == 2))).cuda()
            assert (got[0][:, dead] == 0).all()                                   # null and empty windows: exactly 0
            if name == "interleaved":
                assert (got[0, 0] == 0).all()                                     # the empty period totals 0
            if di != si % 3:                                                      # (transforms: one day vector per structure)
                continue
            gpoly, st = engine.season_reduce(Xd, rb, rows, doy, win, poly=(KELVIN, 1, 4))
            assert gpoly.shape == (4, P, n) and int(st.item()) == 0
            for k in range(4):
                _ok(gpoly[k].cpu().numpy(), _psum(m01 * fpoly[k], rb, rows), rtol, _psum(m01 * np.abs(fpoly[k]), rb, rows))
            gedd, st = engine.season_reduce(Xd, rb, rows, doy, win, X2=Hd, edd=(KELVIN, thr))
            assert gedd.shape == (3, P, n) and int(st.item()) == 0
            for k in range(3):
                _ok(gedd[k].cpu().numpy(), _psum(m01 * fedd[k], rb, rows), SUM_TOL[dtype], _psum(m01 * np.abs(fedd[k]), rb, rows))
                _rel_ok(gedd[k].cpu().numpy(), _psum(m01 * oedd[k], rb, rows), rtol, scale=0.05 * max(1, T))
            # whatever stands out of season is never looked at
            Xp, Hp = X.copy(), H.copy()
            poison = np.array([np.nan, np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 3]
            Xp[m01 == 0] = poison[m01 == 0]
            Hp[m01 == 0] = poison[m01 == 0]
            Xpd, Hpd = strided(Xp), strided(Hp)
            for kw, want in (({}, got), ({"poly": (KELVIN, 1, 4)}, gpoly), ({"X2": Hpd, "edd": (KELVIN, thr)}, gedd)):
                g2, st = engine.season_reduce(Xpd, rb, rows, doy, win, **kw)
                assert torch.equal(g2, want) and int(st.item()) == 0, (name, dname, sorted(kw))
        # windows open all year: the period kernel's result, bit for bit
        doy = _doys(T)[si % 3][1]
        for kw in ({}, {"poly": (KELVIN, 1, 4)}, {"X2": Hd, "edd": (KELVIN, thr)}):
            a, sa = engine.season_reduce(Xd, rb, rows, doy, open_all, **kw)
            b, sb = engine.period_reduce(Xd, rb, rows, **kw)
            assert torch.equal(a, b) and int(sa.item()) == int(sb.item()) == 0, (name, sorted(kw))
    # one in-season +inf: bit 0 (cell 0 is open all year; row 0 is in every structure's first non-empty period)
    Xi = X.copy()
    Xi[0, 0] = np.inf
    doy = _doys(T)[0][1]
    z1, z2 = _mixed_cells(n, doy)
    got, st = engine.season_reduce(strided(Xi), [0, T], np.arange(T), doy, _pack(z1, z2))
    assert int(st.item()) == 1 and torch.isinf(got[0, 0, 0])


def test_kernel_arguments_are_checked(torch_cuda):
    """doy / windows of the wrong length or type and bad row lists are refused; a day outside 0..1023 is in no season; the
    library refuses the keep-NaN flag."""
    import ctypes as C
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    X = torch.full((9, 63), 2.0, dtype=torch.float32, device="cuda")
    rb, rows, doy, win = [0, 9], np.arange(9), np.arange(1, 10), np.full(63, OPEN, dtype=np.int32)
    got, st = engine.season_reduce(X, rb, rows, doy, win)
    assert float(got[0, 0, 8]) == 18.0 and int(st.item()) == 0
    odd = doy.copy()
    odd[[0, 4]] = [-3, 1024]
    assert float(engine.season_reduce(X, rb, rows, odd, win)[0][0, 0, 8]) == 14.0
    with pytest.raises(ValueError):
        engine.season_reduce(X, rb, rows, doy[:8], win)
    with pytest.raises(ValueError):
        engine.season_reduce(X, rb, rows, doy, win[:62])
    with pytest.raises(TypeError):
        engine.season_reduce(X, rb, rows, doy.astype(np.float64), win)
    with pytest.raises(ValueError):
        engine.season_reduce(X, [0, 2], [0, 9], doy, win)
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()
    with pytest.raises(_lib.WaggError) as e:
        engine.season_reduce(X, dev([0, 2]), dev([0, 9]), dev(doy), dev(win))
    assert e.value.code == -1 and "row" in str(e.value)
    L = _lib.load()
    out, status = torch.empty((1, 1, 63), dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [p(X), None, 9, 63, 63, p(dev(rb)), p(dev(rows)), 1, 9, p(dev(doy)), p(dev(win)), _lib.XF_NONE, 0.0, 1, 1, None, 0]
    tail = [p(out), 63, 63, p(status), None, 0, None]
    assert L.wagg_season_reduce_f32(*args, _lib.PERIOD_KEEP_NAN, *tail) == -1 and b"flags" in L.wagg_last_error()
    assert L.wagg_season_reduce_f32(*args[:9], None, args[10], *args[11:], 0, *tail) == -1 and b"doy" in L.wagg_last_error()


def test_materialised_mask_equals_the_restatement(torch_cuda):
    """engine.season_mask and SeasonMask.values: exactly the reference's mask, NaN placement included."""
    from climate_toolbox_amd import engine, get_daily_growing_season_mask
    from tests.test_seasons_host import CELLS, growing_days
    doy = np.concatenate([np.arange(1, 367), [0, 1023]])
    z1, z2 = _mixed_cells(50, np.arange(90, 130))
    win = _pack(z1, z2)
    got = engine.season_mask(doy, win).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (50, 368)
    np.testing.assert_array_equal(got, ref_mask(z1, z2, doy))
    out = engine.season_mask(np.array([-1, 1024, 5000]), win).cpu().numpy()       # days a window cannot hold: in no season
    np.testing.assert_array_equal(out, np.where(np.isnan(z1)[:, None], np.nan, np.zeros((50, 3))))
    ds, gz1, gz2, lat, lon = growing_days(CELLS)
    time = np.arange("2003-12-20", "2005-01-10", dtype="datetime64[D]")           # all of the leap year 2004
    m = get_daily_growing_season_mask(lat, lon, time, ds)
    from climate_toolbox_amd import day_of_year
    want = ref_mask(gz1.reshape(-1), gz2.reshape(-1), day_of_year(time)).reshape(gz1.shape + (len(time),))
    vals = m.values
    assert vals.dtype == np.float64 and vals.shape == m.shape
    np.testing.assert_array_equal(vals, want)


# ---------------------------------------------------------------------------------------------------------------------
# the public calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["segment", "dense"])
def plan_kind(request, monkeypatch):
    """Which family serves the table, forced the way tests/test_gpu_periods.py forces it."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _plans
    pkg.clear_caches()
    dense = request.param == "dense"
    monkeypatch.setattr(_plans, "_wants_dense", lambda n_ucells, G, layout, **k: dense and layout == "TG")
    yield request.param
    pkg.clear_caches()


def _seasons_for(c, seed, extra_lat=1):
    """A growing-days Dataset covering the case's grid (its longitudes labelled 0..360-style: the case's + 180; one more row of
    latitudes than the case has) and the (nlat, nlon) z1 / z2 planes on the case's own cells.  Days sit around 1..70 and the
    year end: plain intervals, wrapping ones, single days, non-integer days, missing planting or harvest days."""
    from climate_toolbox_amd import minixr
    rng = np.random.default_rng(seed)
    nlat, nlon = c.nlat + extra_lat, c.nlon
    z1 = rng.integers(1, 45, (nlat, nlon)).astype(np.float64)
    z2 = z1 + rng.integers(0, 40, (nlat, nlon))
    kind = rng.integers(0, 8, (nlat, nlon))
    wrap = kind == 1
    z1[wrap], z2[wrap] = rng.integers(340, 366, wrap.sum()), rng.integers(2, 30, wrap.sum())
    z1[kind == 2] = np.nan
    z2[kind == 3] = np.nan
    z1[kind == 4] += 0.5
    z2[kind == 4] += 0.25
    lat = np.concatenate([c.lat, c.lat[-1] + 0.5 * np.arange(1, extra_lat + 1)])
    order = rng.permutation(nlon)                                                 # the file's longitudes are not sorted
    ds = minixr.Dataset({"variable": (("z", "latitude", "longitude"), np.stack([z1, z2])[:, :, order])},
                        coords={"z": np.array([1, 2]), "latitude": lat, "longitude": (c.lon + 180.0)[order]})
    return ds, z1[:c.nlat], z2[:c.nlat]


def _mask_TG(z1, z2, doy):
    """(T, G) mask of the case's cells, row-major (lat, lon): 0 / 1 / NaN"""
    return ref_mask(z1.reshape(-1), z2.reshape(-1), doy).T


def _oracle(c, masked, rb, rows):
    from oracle import ref_numpy as O
    daily = O.agg_coded(masked, c.cell, c.code, c.w_eff, c.R)
    with np.errstate(invalid="ignore"):
        absd = O.agg_coded(np.abs(np.nan_to_num(masked, nan=0.0, posinf=0.0, neginf=0.0)), c.cell, c.code, c.w_eff, c.R)
    return _psum(daily, rb, rows), _psum(absd, rb, rows)


@pytest.mark.parametrize("nlat,nlon,T,R,dtype", [(16, 16, 70, 40, np.float32), (7, 9, 9, 5, np.float64)])
def test_season_totals_match_the_oracle(torch_cuda, plan_kind, monkeypatch, nlat, nlon, T, R, dtype):
    """A plain variable, powers 1..4 in one call, snyder_edd and snyder_gdd with season=, on device-resident fields, for a
    label array with dropped rows: the oracle on the daily field masked in NumPy, summed per period.  The plain variable
    also against the existing period call on a host-premasked field; the region without weight is NaN in both; the kernel
    that ran is wagg_season_reduce_*; the plan kind that served the call is the one asked for."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, periods
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, snyder_edd, snyder_gdd, tas_poly_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Case(nlat, nlon, T, R, dtype, seed=nlat + T + R + 1)
    gd, z1, z2 = _seasons_for(c, seed=T)
    sw = pkg.season_windows(gd)
    calls, pcalls, real, real_p = [], [], engine.season_reduce, engine.period_reduce
    monkeypatch.setattr(engine, "season_reduce", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(engine, "period_reduce", lambda *a, **k: pcalls.append(1) or real_p(*a, **k))
    lab = np.arange(T) % 3
    lab[1::4] = -1
    labels, rb, rows = periods.period_rows(c.time, lab)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time))
    assert np.isnan(mask).any() and (mask == 0).any() and (mask == 1).any()
    cmin, cmax = c.tas + dtype(KELVIN), c.tasmax + dtype(KELVIN)
    e_own, e_max = float(cmin[0, 0, 1]), float(cmax[0, 0, 2])
    ds = c.dataset(torch, tas=c.tas, tasmin=c.tas, tasmax=c.tasmax)
    for k in ("tasmin", "tasmax"):
        ds[k].attrs["units"] = "K"
        ds = convert_kelvin_to_celsius(ds, k)
    ds["edd"] = snyder_edd(ds.tasmin, ds.tasmax, e_own)
    ds["gdd"] = snyder_gdd(ds.tasmin, ds.tasmax, 10, e_max)
    fields = {"tas": c.tas, "edd": O.snyder_edd_values(cmin, cmax, e_own), "gdd": O.snyder_gdd_values(cmin, cmax, 10, e_max)}
    for name, f in fields.items():
        ref, absref = _oracle(c, mask * np.asarray(f).reshape(T, c.G), rb, rows)
        if name != "tas":
            absref = np.maximum(absref, 0.05 * max(1, T))        # (the fp32 degree-day polynomial: 2e-6 absolute per value)
        del calls[:]
        out = pkg.weighted_aggregate_grid_to_regions_periods(ds, name, "popwt", "reg", c.df, period=lab, season=sw)
        assert calls == [1] and pcalls == []                     # one route: wagg_season_reduce_*, never a period route
        assert out[name].dims == ("period", "reg") and "time" not in out.coords
        np.testing.assert_array_equal(out["period"].values, labels)
        got = out[name].values
        assert got.dtype == dtype and np.isnan(got[:, R - 1]).all() and np.isnan(ref[:, R - 1]).all()
        _ok(got, ref, c.rtol, absref)
        if name == "tas":                                         # ... and what a caller had to do before: mask on the host
            pre = np.where(mask == 1, c.tas.reshape(T, c.G), dtype(0)).astype(dtype).reshape(c.tas.shape)
            old = pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch, device=False, tas=pre), "tas", "popwt", "reg", c.df,
                                                                 period=lab)
            assert pcalls and calls == [1]
            del pcalls[:]
            assert np.isnan(old.tas.values[:, R - 1]).all()
            _ok(got, old.tas.values, c.rtol, absref)
    # powers 1..4 in one pass; tas_poly_aggregate relabels the days to YYYYDDD, here the same days of year
    del calls[:]
    out = tas_poly_aggregate(c.dataset(torch), [1, 2, 3, 4], "popwt", "reg", c.df, period=lab, season=sw)
    assert calls == [1] and pcalls == []
    for p in (1, 2, 3, 4):
        ref, absref = _oracle(c, mask * O.tas_poly_values(c.tas, p).reshape(T, c.G), rb, rows)
        assert out["tas-poly-%d" % p].dims == ("period", "reg")
        _ok(out["tas-poly-%d" % p].values, ref, c.rtol, absref)
    from climate_toolbox_amd._plans import _PLAN_CACHE
    kinds = {type(p).__name__ for p in _PLAN_CACHE.values()}
    assert kinds == ({"DensePlan"} if plan_kind == "dense" else {"SparsePlan"}), kinds


def test_layouts_residency_years_and_device_results(torch_cuda, plan_kind):
    """period="year" over two years (the days of year run across the year end) on: a device-resident (time, lat, lon) field, a
    SeasonMask instead of the windows, a host-resident field, a (lat, lon, time) field, a dataset standardised from a file whose
    0..360 longitudes are not in ascending order (its buffer stays in file order), and under results_on_device()."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import minixr, periods
    torch = torch_cuda
    T = 70
    c = _Case(7, 9, T, 5, np.float32, seed=31)
    c.time = np.datetime64("2003-12-01") + np.arange(T)                           # 31 days of 2003, 39 of 2004
    gd, z1, z2 = _seasons_for(c, seed=5, extra_lat=2)
    sw = pkg.season_windows(gd)
    labels, rb, rows = periods.period_rows(c.time, "year")
    assert list(labels) == [2003, 2004]
    doy = pkg.day_of_year(c.time)
    assert doy[30] == 365 and doy[31] == 1
    ref, absref = _oracle(c, _mask_TG(z1, z2, doy) * c.tas.reshape(T, c.G), rb, rows)
    call = lambda ds, season=sw: pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "reg", c.df, period="year", season=season)
    dev = call(c.dataset(torch))
    assert dev.tas.dims == ("period", "reg") and isinstance(dev.tas.data, np.ndarray)
    _ok(dev.tas.values, ref, c.rtol, absref)
    mask = pkg.get_daily_growing_season_mask(c.lat, c.lon, np.arange(3), gd)      # its own time is not what counts: the dataset's is
    np.testing.assert_array_equal(call(c.dataset(torch), mask).tas.values, dev.tas.values)
    host = call(c.dataset(torch, device=False))
    assert isinstance(host.tas.data, np.ndarray)
    np.testing.assert_array_equal(host.tas.values, dev.tas.values)                # the same kernels on the same numbers
    gt = minixr.Dataset({"tas": (("lat", "lon", "time"), torch.from_numpy(np.ascontiguousarray(np.moveaxis(c.tas, 0, -1))).cuda())},
                        coords={"time": c.time, "lat": c.lat, "lon": c.lon})
    out = call(gt)
    assert out.tas.dims == ("reg", "period")
    np.testing.assert_array_equal(out.tas.values.T, dev.tas.values)
    gt_host = minixr.Dataset({"tas": (("lat", "lon", "time"), np.ascontiguousarray(np.moveaxis(c.tas, 0, -1)))},
                             coords={"time": c.time, "lat": c.lat, "lon": c.lon})
    np.testing.assert_array_equal(call(gt_host).tas.values.T, dev.tas.values)
    roll = np.roll(np.arange(c.nlon), 4)                                          # a file that starts in the middle of the axis
    raw = minixr.Dataset({"tas": (("time", "lat", "lon"), torch.from_numpy(np.ascontiguousarray(c.tas[:, :, roll])).cuda())},
                         coords={"time": c.time, "lat": c.lat, "lon": c.lon[roll]})
    std = pkg.standardize_climate_data(raw)
    assert getattr(std["tas"], "_lon_perm", None) is not None and list(std.coords["lon"].values) == list(c.lon)
    _ok(call(std).tas.values, ref, c.rtol, absref)              # (another cell order in the plan: not the same bits)
    with pkg.results_on_device():
        on = call(c.dataset(torch))
        assert isinstance(on.tas.data, torch.Tensor) and on.tas.data.is_cuda and tuple(on.tas.data.shape) == (2, 5)
    np.testing.assert_array_equal(on.tas.values, dev.tas.values)
    four_d = minixr.Dataset({"tas": (("time", "lev", "lat", "lon"), np.zeros((T, 2, c.nlat, c.nlon), dtype=np.float32))},
                            coords={"time": c.time, "lat": c.lat, "lon": c.lon})
    with pytest.raises(ValueError, match="time"):
        call(four_d)


def test_in_season_inf_and_missing_cells_raise(torch_cuda, plan_kind):
    """+-inf out of season is nobody's business; in season it raises ValueError (no daily route exists to give it the daily
    treatment); a dataset cell that the mask's grid lacks raises KeyError."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import minixr
    torch = torch_cuda
    c = _Case(7, 9, 9, 5, np.float64, seed=3)
    gd, z1, z2 = _seasons_for(c, seed=8)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time)).reshape(c.T, c.nlat, c.nlon)
    call = lambda ds, season=sw: pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "reg", c.df, period="year", season=season)
    clean = call(c.dataset(torch)).tas.values
    t, i, j = [int(v[0]) for v in np.nonzero(mask == 0)]
    c.tas[t, i, j] = np.inf
    nt, ni, nj = [int(v[0]) for v in np.nonzero(np.isnan(mask))]
    c.tas[nt, ni, nj] = -np.inf
    np.testing.assert_array_equal(call(c.dataset(torch)).tas.values, clean)
    t, i, j = [int(v[0]) for v in np.nonzero(mask == 1)]
    keep = c.tas[t, i, j]
    for bad in (np.inf, -np.inf):
        c.tas[t, i, j] = bad
        with pytest.raises(ValueError, match="inf"):
            call(c.dataset(torch))
    c.tas[t, i, j] = keep
    np.testing.assert_array_equal(call(c.dataset(torch)).tas.values, clean)
    short = pkg.SeasonWindows(sw.windows[:, 1:], sw.latitude, sw.longitude[1:])     # the mask's grid lacks one longitude
    with pytest.raises(KeyError):
        call(c.dataset(torch), short)
    with pytest.raises(TypeError):
        call(c.dataset(torch), np.zeros((7, 9)))
