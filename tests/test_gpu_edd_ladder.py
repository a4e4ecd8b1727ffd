"""Degree-day ladders on the GPU (run with -m gpu): wagg_edd_ladder_reduce_* through engine.edd_ladder_reduce against the
four-plane kernels it must equal bit for bit (engine.season_reduce / engine.period_reduce, themselves pinned to the oracle by
tests/test_gpu_seasons.py and tests/test_gpu_periods.py) and against the oracle directly, and snyder_edd_aggregate on both plan
kinds against the single calls -- at the shapes, windows and period structures of those two files."""
import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok
from tests.test_gpu_periods import SUM_TOL, _Case, _field, _ok, _psum, _structures
from tests.test_gpu_seasons import KELVIN, _doys, _mask_TG, _mixed_cells, _oracle, _pack, _seasons_for, plan_kind  # noqa: F401
from tests.test_seasons_host import ref_mask

pytestmark = pytest.mark.gpu

A_MIN, A_MAX, A_FLAT = 12, 18, 24               # open-all-year cells (j % 6 == 0) whose row-0 values become thresholds


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _grouped(call, thr, order):
    """the planes of ``thr`` from calls of up to four thresholds each, the thresholds taken in ``order``"""
    planes = [None] * len(thr)
    for g in range(0, len(order), 4):
        idx = order[g:g + 4]
        got, st = call([thr[i] for i in idx])
        assert int(st.item()) == 0
        for pos, i in enumerate(idx):
            planes[i] = got[pos]
    return planes


@pytest.mark.parametrize("dtype,rtol", [(np.float32, RTOL32), (np.float64, RTOL64)])
@pytest.mark.parametrize("n,pad", [(63, 0), (63, 3), (1100, 0), (1100, 3)])
@pytest.mark.parametrize("T", [9, 70])
def test_ladder_planes_equal_the_four_plane_kernels_and_the_oracle(torch_cuda, dtype, rtol, n, pad, T):
    """Every plane of ladders of 1, 4, 5, G, G + 1, 17 and 64 thresholds equals, bit for bit, the plane engine.season_reduce
    gives for that threshold in two different groups of four -- under mixed windows (null, empty, single-day, wrapping, open)
    -- and without a season the plane of engine.period_reduce; for every period structure (T = 70 with one period: the split
    path; "interleaved": an empty period).  The thresholds: below every tasmin, above every tasmax, a cell's own tasmin, a
    cell's own tasmax, the value of a cell with tasmin == tasmax, and 59 across the range.  Two runs are bit-equal, the status
    word is 0, null / empty windows and the empty period total exactly 0 in all 64 planes, a NaN tasmin in season counts 0 in
    every plane; NaN, +inf and 1e30 out of season change no bit and no status; one in-season +inf in tasmax sets bit 0.
    Against the oracle: the tolerances of tests/test_gpu_seasons.py::test_kernel_sums_match_numpy."""
    from climate_toolbox_amd import _lib, engine
    from climate_toolbox_amd.periods import period_rows
    from oracle import ref_numpy as O
    torch = torch_cuda
    G = _lib.EDD_LADDER_GROUP
    rng = np.random.default_rng(100 * T + n + pad)
    Xd, X = _field(rng, T, n, pad, dtype, torch)
    H = (X + rng.uniform(0, 12, X.shape)).astype(dtype)
    H[0, A_FLAT] = X[0, A_FLAT]                         # a day without a diurnal range

    def strided(host):
        buf = torch.zeros((T, n + pad), dtype=Xd.dtype, device="cuda")
        buf[:, :n] = torch.from_numpy(host).cuda()
        return buf[:, :n]

    X[0, 0] = np.nan                                    # (cell 0 is open all year: NaN in season)
    X[:, 6] = np.nan                                    # NaN tasmin on every day, in a cell that is open all year
    Xd, Hd = strided(X), strided(H)
    assert Xd.stride(0) == n + pad
    cmin, cmax = X + dtype(KELVIN), H + dtype(KELVIN)
    special = [float(np.nanmin(cmin)) - 5.0, float(np.nanmax(cmax)) + 5.0, float(cmin[0, A_MIN]), float(cmax[0, A_MAX]),
               float(cmin[0, A_FLAT])]
    thr = list(np.linspace(-35.0, 52.0, 59)) + special
    thr = [thr[i] for i in np.random.default_rng(7).permutation(64)]              # (a ladder need not ascend)
    assert len(set(thr)) == 64
    sizes = sorted({1, 4, 5, G, G + 1, 17, 64})
    assert len(sizes) == 7
    orders = [list(range(64)), list(np.roll(np.arange(64)[::-1], 2))]            # every threshold in two different groups of four
    assert all(set(orders[0][4 * (i // 4):4 * (i // 4) + 4]) != set(orders[1][4 * (orders[1].index(i) // 4):][:4]) for i in range(64))
    fedd = np.stack([np.nan_to_num(engine.transform_edd(Xd, Hd, KELVIN, [(1.0, e)]).cpu().numpy(), nan=0.0) for e in thr], axis=1)
    oedd = np.stack([np.nan_to_num(O.snyder_edd_values(cmin, cmax, e), nan=0.0) for e in thr], axis=1)      # (T, 64, n)
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
        full, st = engine.edd_ladder_reduce(Xd, Hd, rb, rows, KELVIN, thr, doy=doy, windows=win)
        assert full.shape == (64, P, n) and int(st.item()) == 0
        again, _ = engine.edd_ladder_reduce(Xd, Hd, rb, rows, KELVIN, thr, doy=doy, windows=win)
        assert torch.equal(again, full)                                           # bit-reproducible
        for order in orders:
            ref = _grouped(lambda g: engine.season_reduce(Xd, rb, rows, doy, win, X2=Hd, edd=(KELVIN, g)), thr, order)
            for k in range(64):
                assert torch.equal(full[k], ref[k]), (name, dname, k, thr[k])
        for m in sizes[:-1]:                                                      # shorter ladders: other groups, a ragged last one
            part, st = engine.edd_ladder_reduce(Xd, Hd, rb, rows, KELVIN, thr[:m], doy=doy, windows=win)
            assert part.shape == (m, P, n) and int(st.item()) == 0 and torch.equal(part, full[:m]), (name, m)
        assert (full[:, :, dead] == 0).all()                                      # null and empty windows: exactly 0, all 64 planes
        assert (full[:, :, 6] == 0).all()                                         # S6: NaN tasmin on every day counts 0 in every plane
        if name == "interleaved":
            assert (full[:, 0] == 0).all()                                        # the empty period totals 0
        # the oracle, masked and period-summed on the host
        got = np.moveaxis(full.cpu().numpy(), 0, 1)                               # (P, 64, n)
        mk = m01[:, None, :]
        _ok(got, _psum(mk * fedd, rb, rows), SUM_TOL[dtype], _psum(mk * np.abs(fedd), rb, rows))
        _rel_ok(got, _psum(mk * oedd, rb, rows), rtol, scale=0.05 * max(1, T))
        # whatever stands out of season is never looked at
        Xp, Hp = X.copy(), H.copy()
        poison = np.array([np.nan, np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 3]
        Xp[m01 == 0] = poison[m01 == 0]
        Hp[m01 == 0] = poison[m01 == 0]
        g2, st = engine.edd_ladder_reduce(strided(Xp), strided(Hp), rb, rows, KELVIN, thr, doy=doy, windows=win)
        assert torch.equal(g2, full) and int(st.item()) == 0, (name, dname)
        # no season: the period kernel's planes, bit for bit
        flat, st = engine.edd_ladder_reduce(Xd, Hd, rb, rows, KELVIN, thr)
        assert flat.shape == (64, P, n) and int(st.item()) == 0
        for order in orders:
            ref = _grouped(lambda g: engine.period_reduce(Xd, rb, rows, X2=Hd, edd=(KELVIN, g)), thr, order)
            for k in range(64):
                assert torch.equal(flat[k], ref[k]), (name, "no season", k, thr[k])
        for m in (5, G + 1):
            part, _ = engine.edd_ladder_reduce(Xd, Hd, rb, rows, KELVIN, thr[:m])
            assert torch.equal(part, flat[:m])
        _rel_ok(np.moveaxis(flat.cpu().numpy(), 0, 1), _psum(oedd, rb, rows), rtol, scale=0.05 * max(1, T))
    # one in-season +inf in tasmax: bit 0 (cell 0 is open all year; row 0 is listed)
    Hi = H.copy()
    Hi[0, 0] = np.inf
    doy = _doys(T)[0][1]
    z1, z2 = _mixed_cells(n, doy)
    _, st = engine.edd_ladder_reduce(strided(np.nan_to_num(X, nan=280.0)), strided(Hi), [0, T], np.arange(T), KELVIN, thr, doy=doy,
                                     windows=_pack(z1, z2))
    assert int(st.item()) == 1
    _, st = engine.edd_ladder_reduce(strided(np.nan_to_num(X, nan=280.0)), strided(Hi), [0, T], np.arange(T), KELVIN, thr)
    assert int(st.item()) == 1


def test_binding_refuses_what_the_library_would(torch_cuda):
    from climate_toolbox_amd import engine
    torch = torch_cuda
    X = torch.full((9, 63), 2.0, dtype=torch.float32, device="cuda")
    H = X + 4.0
    rb, rows, doy, win = [0, 9], np.arange(9), np.arange(1, 10), np.full(63, 1023 << 10, dtype=np.int32)
    got, st = engine.edd_ladder_reduce(X, H, rb, rows, 0.0, [1.0, 9.0], doy=doy, windows=win)
    assert got.shape == (2, 1, 63) and float(got[0, 0, 5]) == 27.0 and float(got[1, 0, 5]) == 0.0 and int(st.item()) == 0
    with pytest.raises(ValueError, match="thresholds"):
        engine.edd_ladder_reduce(X, H, rb, rows, 0.0, list(range(65)))
    with pytest.raises(ValueError, match="thresholds"):
        engine.edd_ladder_reduce(X, H, rb, rows, 0.0, [])
    with pytest.raises(ValueError, match="go together"):
        engine.edd_ladder_reduce(X, H, rb, rows, 0.0, [1.0], doy=doy)
    with pytest.raises(ValueError):
        engine.edd_ladder_reduce(X, H[:8], rb, rows, 0.0, [1.0])
    with pytest.raises(ValueError):
        engine.edd_ladder_reduce(X, H, rb, rows, 0.0, [1.0], doy=doy[:8], windows=win)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_public_call(torch_cuda, plan_kind, monkeypatch, dtype):
    """snyder_edd_aggregate with nine thresholds, period="year" over a year end and a season: bit for bit the nine single calls
    on snyder_edd variables (same route, plan and row order), the oracle within the tolerances of
    tests/test_gpu_seasons.py::test_season_totals_match_the_oracle; dims, refTemp and units; period=None = the stacked daily
    single calls; (lat, lon, time) and host-resident fields; 70 thresholds in two slices; results_on_device().  The period
    route is engine.edd_ladder_reduce, once per 64 thresholds, and never the four-plane reductions; the daily route is neither."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, minixr, periods
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, snyder_edd, snyder_edd_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    T, R = 9, 5
    c = _Case(7, 9, T, R, dtype, seed=23)
    c.time = np.datetime64("2003-12-27") + np.arange(T)                           # 5 days of 2003, 4 of 2004
    gd, z1, z2 = _seasons_for(c, seed=T)
    sw = pkg.season_windows(gd)
    labels, rb, rows = periods.period_rows(c.time, "year")
    assert list(labels) == [2003, 2004]
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time))
    assert np.isnan(mask).any() and (mask == 0).any() and (mask == 1).any()
    cmin, cmax = c.tas + dtype(KELVIN), c.tasmax + dtype(KELVIN)
    thr = [-40.0, 60.0, float(cmin[0, 0, 1]), float(cmax[0, 0, 2]), 0.0, 8.0, 10.5, 19.0, 30.0]

    def celsius(ds):
        for k in ("tasmin", "tasmax"):
            ds[k].attrs["units"] = "K"
            ds = convert_kelvin_to_celsius(ds, k)
        return ds

    def dataset(device=True, moved=False):
        if not moved:
            return celsius(c.dataset(torch, device=device, tasmin=c.tas, tasmax=c.tasmax))
        wrap = (lambda v: torch.from_numpy(v).cuda()) if device else (lambda v: v)
        return celsius(minixr.Dataset({k: (("lat", "lon", "time"), wrap(np.ascontiguousarray(np.moveaxis(v, 0, -1))))
                                       for k, v in (("tasmin", c.tas), ("tasmax", c.tasmax))},
                                      coords={"time": c.time, "lat": c.lat, "lon": c.lon}))

    ran = {"edd_ladder_reduce": 0, "season_reduce": 0, "period_reduce": 0}
    for name in ran:
        def counted(*a, _name=name, _real=getattr(engine, name), **k):
            ran[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(engine, name, counted)

    def launches():
        """(ladder launches, four-plane reductions) since the last look"""
        got = (ran["edd_ladder_reduce"], ran["season_reduce"] + ran["period_reduce"])
        ran.update(dict.fromkeys(ran, 0))
        return got

    call = lambda ds, t=thr, **kw: snyder_edd_aggregate(ds, t, "popwt", "reg", c.df, **kw)
    out = call(dataset(), period="year", season=sw)
    assert launches() == (1, 0)                                                   # nine thresholds: one launch, nothing grouped
    assert out["edd"].dims == ("refTemp", "period", "reg") and out["edd"].attrs["units"] == "degreedays_C"
    assert out["refTemp"].values.dtype == np.float64 and list(out["refTemp"].values) == thr
    np.testing.assert_array_equal(out["period"].values, labels)
    got = out["edd"].values
    assert got.shape == (9, 2, R) and got.dtype == dtype and isinstance(out["edd"].data, np.ndarray)
    ds = dataset()
    for k, e in enumerate(thr):
        ds["one"] = snyder_edd(ds.tasmin, ds.tasmax, e)
        single = pkg.weighted_aggregate_grid_to_regions_periods(ds, "one", "popwt", "reg", c.df, period="year", season=sw)
        np.testing.assert_array_equal(got[k], single["one"].values, err_msg="threshold %r" % e)
        ref, absref = _oracle(c, mask * np.asarray(O.snyder_edd_values(cmin, cmax, e)).reshape(T, c.G), rb, rows)
        assert np.isnan(got[k][:, R - 1]).all() and np.isnan(ref[:, R - 1]).all()
        _ok(got[k], ref, c.rtol, np.maximum(absref, 0.05 * max(1, T)))
    other = call(dataset(), varname="dd", period="year", season=sw, tasmin="tasmin", tasmax="tasmax")
    np.testing.assert_array_equal(other["dd"].values, got)
    # no season: the plain period totals, against the oracle
    launches()
    plain = call(dataset(), period="year")["edd"].values
    assert launches() == (1, 0)
    for k, e in enumerate(thr):
        ref, absref = _oracle(c, np.asarray(O.snyder_edd_values(cmin, cmax, e)).reshape(T, c.G), rb, rows)
        _ok(plain[k], ref, c.rtol, np.maximum(absref, 0.05 * max(1, T)))
    # daily results: the stacked single calls, bit for bit
    daily = call(dataset())
    assert launches() == (0, 0)                                                   # (the fused daily apply, four thresholds a pass)
    assert daily["edd"].dims == ("refTemp", "time", "reg") and daily["edd"].values.shape == (9, T, R)
    np.testing.assert_array_equal(daily["time"].values, c.time)
    for k, e in enumerate(thr):
        ds["one"] = snyder_edd(ds.tasmin, ds.tasmax, e)
        single = pkg.weighted_aggregate_grid_to_regions(ds, "one", "popwt", "reg", c.df)
        np.testing.assert_array_equal(daily["edd"].values[k], single["one"].values, err_msg="daily, threshold %r" % e)
    np.testing.assert_array_equal(call(dataset(device=False))["edd"].values, daily["edd"].values)
    # other layouts and residencies: the same kernels on the same numbers
    launches()
    np.testing.assert_array_equal(call(dataset(device=False), period="year", season=sw)["edd"].values, got)
    assert launches() == (1, 0)
    moved = call(dataset(moved=True), period="year", season=sw)
    assert moved["edd"].dims == ("refTemp", "reg", "period")
    np.testing.assert_array_equal(np.swapaxes(moved["edd"].values, 1, 2), got)
    np.testing.assert_array_equal(np.swapaxes(call(dataset(device=False, moved=True), period="year", season=sw)["edd"].values, 1, 2), got)
    # 70 thresholds: two launches, joined in the caller's order
    many = list(np.linspace(-20.0, 49.0, 70))
    launches()
    out70 = call(dataset(), many, period="year", season=sw)
    assert launches() == (2, 0)                                                   # 64 + 6
    assert out70["edd"].values.shape == (70, 2, R) and list(out70["refTemp"].values) == many
    pick = [0, 1, 62, 63, 64, 65, 69]
    np.testing.assert_array_equal(out70["edd"].values[pick], call(dataset(), [many[i] for i in pick], period="year", season=sw)["edd"].values)
    with pkg.results_on_device():
        on = call(dataset(), period="year", season=sw)
        assert isinstance(on["edd"].data, torch.Tensor) and on["edd"].data.is_cuda and tuple(on["edd"].data.shape) == (9, 2, R)
        on_daily = call(dataset())
        assert isinstance(on_daily["edd"].data, torch.Tensor) and on_daily["edd"].data.is_cuda
        assert isinstance(call(dataset(device=False))["edd"].data, np.ndarray)    # (a host-resident field's result is a host array)
    np.testing.assert_array_equal(on["edd"].values, got)
    np.testing.assert_array_equal(on_daily["edd"].values, daily["edd"].values)


def test_public_call_in_season_inf_raises(torch_cuda, plan_kind):
    """+inf out of season is nobody's business; in season it raises ValueError -- in tasmax alone, or in both fields (a tasmin
    above its tasmax is refused earlier, like the reference refuses it)."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd.transformations import snyder_edd_aggregate
    torch = torch_cuda
    c = _Case(7, 9, 9, 5, np.float64, seed=3)
    gd, z1, z2 = _seasons_for(c, seed=8)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time)).reshape(c.T, c.nlat, c.nlon)
    thr = [270.0, 285.0, 290.0, 300.0, 310.0]                                    # (the fields stay in Kelvin: plain fields)

    def call():
        return snyder_edd_aggregate(c.dataset(torch, tasmin=c.tas, tasmax=c.tasmax), thr, "popwt", "reg", c.df, period="year", season=sw)

    clean = call()["edd"].values
    t, i, j = [int(v[0]) for v in np.nonzero(mask == 0)]
    c.tasmax[t, i, j] = np.inf
    nt, ni, nj = [int(v[0]) for v in np.nonzero(np.isnan(mask))]
    c.tas[nt, ni, nj] = -np.inf
    np.testing.assert_array_equal(call()["edd"].values, clean)
    t, i, j = [int(v[0]) for v in np.nonzero(mask == 1)]
    keep_max, keep_min = c.tasmax[t, i, j], c.tas[t, i, j]
    c.tasmax[t, i, j] = np.inf
    with pytest.raises(ValueError, match="inf"):
        call()
    c.tas[t, i, j] = np.inf
    with pytest.raises(ValueError, match="inf"):
        call()
    c.tasmax[t, i, j], c.tas[t, i, j] = keep_max, keep_min
    np.testing.assert_array_equal(call()["edd"].values, clean)
