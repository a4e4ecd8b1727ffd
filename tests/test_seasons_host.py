"""Growing-season windows, the part that needs no GPU (climate_toolbox_amd/seasons.py): season_boundaries, the packed windows,
the day of year and the argument errors, against a brute-force NumPy restatement of the reference's mask
(climate_toolbox/utils/utils.py:83-153) written here on plain arrays -- never by calling seasons.py."""
import numpy as np
import pytest

NAN = np.nan
# (planting day z1, harvest day z2) of the cells every test here looks at
CELLS = [(100, 200),          # z2 > z1: a plain interval
         (300, 100),          # z2 < z1: the season wraps the year end; days 100 and 300 themselves are out
         (150, 150),          # z2 == z1: a single day
         (NAN, 200),          # no planting day: the mask is NaN
         (NAN, NAN),
         (50, NAN),           # no harvest day: d <= NaN never holds, the complement is the whole year
         (120.5, 300.25),     # non-integer days
         (300.25, 120.5),
         (-5, 40),            # days <= 0
         (0, 10),
         (40, -5),
         (-10, -3),
         (200, 400),          # days > 366
         (400, 200),
         (2000, 3000),        # beyond what a window can hold: nothing / everything
         (3000, 2000)]


def ref_mask(z1, z2, doy):
    """utils.py:143-149 on plain arrays: ``z1`` / ``z2`` (n,), ``doy`` (T,) -> the (n, T) mask, 0 / 1 / NaN"""
    z1, z2, d = np.asarray(z1, dtype=np.float64), np.asarray(z2, dtype=np.float64), np.asarray(doy, dtype=np.float64)[None, :]
    both = np.sort(np.stack([z1, z2], axis=-1), axis=-1)                     # season_boundaries: NaN last
    with np.errstate(invalid="ignore"):
        mask = (d >= both[:, :1]) & (d <= both[:, 1:])                         # dayofyear >= min_day, <= max_day
        final = np.where((z2 >= z1)[:, None], mask.astype(np.float64), NAN)    # .where(z2 >= z1)
    final = np.where(np.isnan(final), 1.0 - mask, final)                       # .fillna(1 - mask)
    return np.where(~np.isnan(z1)[:, None], final, NAN)                        # .where(~z1.isnull())


def decode(win, doy):
    """the packing of include/wagg.h read back: (n,) int32 windows, (T,) days -> the (n, T) mask, 0 / 1 / NaN"""
    win, d = np.asarray(win, dtype=np.int64)[:, None], np.asarray(doy, dtype=np.int64)[None, :]
    a, b, invert, null = win & 1023, (win >> 10) & 1023, (win >> 20) & 1, (win >> 21) & 1
    inside = (d >= a) & (d <= b)
    season = (inside != (invert == 1)) & (d >= 0) & (d <= 1023)
    return np.where(null == 1, NAN, season.astype(np.float64))


def growing_days(cells=CELLS, nlat=2, lon0=180.0):
    """The cells as a growing-days Dataset variable(z, latitude, longitude) whose longitudes run 0..360 and start at
    ``lon0``, so that the -180 shift leaves them unsorted; also the (nlat, nlon) z1 / z2 planes in the SHIFTED, SORTED order."""
    from climate_toolbox_amd import minixr
    z = np.asarray(cells, dtype=np.float64).reshape(nlat, -1, 2)
    nlon = z.shape[1]
    lon = (lon0 + np.arange(nlon) * (360.0 / nlon)) % 360.0
    lat = 10.0 + 0.5 * np.arange(nlat)
    ds = minixr.Dataset({"variable": (("z", "latitude", "longitude"), np.moveaxis(z, 2, 0))},
                        coords={"z": np.array([1, 2]), "latitude": lat, "longitude": lon})
    order = np.argsort(lon - 180.0, kind="stable")
    return ds, z[:, order, 0], z[:, order, 1], lat, (lon - 180.0)[order]


def test_boundaries_are_the_sorted_pair_on_the_shifted_sorted_grid():
    from climate_toolbox_amd import season_boundaries
    ds, z1, z2, lat, lon = growing_days()
    before = np.array(ds.coords["longitude"].values)
    assert (np.diff(before - 180.0) < 0).any()                                 # the shift alone leaves the axis unsorted
    mn, mx = season_boundaries(ds)
    assert mn.dims == mx.dims == ("latitude", "longitude")
    np.testing.assert_array_equal(mn.coords["longitude"], lon)
    np.testing.assert_array_equal(mn.coords["latitude"], lat)
    assert (np.diff(lon) > 0).all() and lon.min() == -180.0
    both = np.sort(np.stack([z1, z2], axis=2), axis=2)
    np.testing.assert_array_equal(mn.values, both[:, :, 0])
    np.testing.assert_array_equal(mx.values, both[:, :, 1])                    # NaN last: (50, NaN) -> min 50, max NaN
    assert mn.values[~np.isnan(mn.values)].size > mx.values[~np.isnan(mx.values)].size
    np.testing.assert_array_equal(ds.coords["longitude"].values, before)       # the caller's dataset is left alone


def test_windows_decode_to_the_reference_mask_on_every_day():
    from climate_toolbox_amd import season_windows
    ds, z1, z2, lat, lon = growing_days()
    sw = season_windows(ds)
    assert sw.windows.dtype == np.int32 and sw.windows.shape == z1.shape
    np.testing.assert_array_equal(sw.longitude, lon)
    np.testing.assert_array_equal(sw.latitude, lat)
    doy = np.arange(1, 367)
    want = ref_mask(z1.reshape(-1), z2.reshape(-1), doy)
    np.testing.assert_array_equal(decode(sw.windows.reshape(-1), doy), want)
    by_cell = {c: want[i] for i, c in enumerate(zip(z1.reshape(-1).tolist(), z2.reshape(-1).tolist()))}
    # the table of the module docstring, spelled out on the oracle itself
    assert by_cell[(100.0, 200.0)].sum() == 101 and by_cell[(150.0, 150.0)].sum() == 1
    wrap = by_cell[(300.0, 100.0)]
    assert wrap[99 - 1] == 1 and wrap[100 - 1] == 0 and wrap[300 - 1] == 0 and wrap[301 - 1] == 1 and wrap.sum() == 366 - 201
    assert by_cell[(120.5, 300.25)].sum() == 300 - 121 + 1 and by_cell[(300.25, 120.5)].sum() == 366 - (300 - 121 + 1)
    assert by_cell[(-5.0, 40.0)].sum() == 40 and by_cell[(40.0, -5.0)].sum() == 366 - 40
    assert by_cell[(2000.0, 3000.0)].sum() == 0 and by_cell[(3000.0, 2000.0)].sum() == 366
    null = np.isnan(z1.reshape(-1))
    assert np.isnan(want[null]).all() and not np.isnan(want[~null]).any()
    assert (want[np.isnan(z2.reshape(-1)) & ~null] == 1).all()                  # no harvest day: in season all year
    # packing details of include/wagg.h: an empty interval is a = 1, b = 0; null is bit 21; the complement is bit 20
    w = {c: int(v) for c, v in zip(zip(z1.reshape(-1).tolist(), z2.reshape(-1).tolist()), sw.windows.reshape(-1).tolist())}
    assert w[(100.0, 200.0)] == 100 | 200 << 10 and w[(300.0, 100.0)] == 100 | 300 << 10 | 1 << 20
    assert w[(2000.0, 3000.0)] == 1 and w[(3000.0, 2000.0)] == 1 | 1 << 20 and w[(-10.0, -3.0)] == 1
    assert w[(-5.0, 40.0)] == 0 | 40 << 10 and w[(200.0, 400.0)] == 200 | 400 << 10
    assert all(v >> 21 == 1 for c, v in w.items() if c[0] != c[0])


def test_windows_from_a_file_and_a_differently_ordered_variable(tmp_path):
    from climate_toolbox_amd import minixr, season_windows
    from climate_toolbox_amd.output import to_netcdf
    ds, *_ = growing_days()
    path = str(tmp_path / "growing_days.nc")
    to_netcdf(ds, path)
    np.testing.assert_array_equal(season_windows(path).windows, season_windows(ds).windows)
    v = ds["variable"]
    flipped = minixr.Dataset({"variable": (("latitude", "longitude", "z"), np.moveaxis(v.values, 0, 2)[:, :, ::-1])},
                             coords={"z": np.array([2, 1]), "latitude": ds.coords["latitude"].values,
                                     "longitude": ds.coords["longitude"].values})
    np.testing.assert_array_equal(season_windows(flipped).windows, season_windows(ds).windows)      # z is selected by label
    with pytest.raises(ValueError):
        season_windows(minixr.Dataset({"variable": (("z", "lat", "lon"), v.values)}))


def test_day_of_year_from_datetime64_and_yyyyddd():
    from climate_toolbox_amd import day_of_year
    t = np.arange("2003-12-30", "2005-01-03", dtype="datetime64[D]")          # across the leap year 2004
    d = day_of_year(t)
    assert d.dtype == np.int32 and list(d[:3]) == [364, 365, 1]
    assert d[2 + 59] == 60 and t[2 + 59] == np.datetime64("2004-02-29")         # 29 February is day 60 ...
    assert list(d[-4:]) == [365, 366, 1, 2]                                     # ... and 2004 has a day 366
    np.testing.assert_array_equal(day_of_year(t.astype("datetime64[ns]")), d)
    np.testing.assert_array_equal(day_of_year(np.array([2001001, 2001059, 2001060, 2001365, 2002001])), [1, 59, 60, 365, 1])
    for bad in (np.arange(3.0), np.array(["a", "b"])):
        with pytest.raises(ValueError):
            day_of_year(bad)


def test_the_mask_object_has_the_references_shape_and_refuses_other_time_types():
    from climate_toolbox_amd import SeasonMask, get_daily_growing_season_mask, minixr
    ds, z1, z2, lat, lon = growing_days()
    time = np.arange("2004-12-25", "2005-01-05", dtype="datetime64[D]")
    m = get_daily_growing_season_mask(np.zeros(3), np.zeros(5), minixr.DataArray(time, ("time",)), ds)    # lat / lon select nothing
    assert isinstance(m, SeasonMask) and m.dims == ("lat", "lon", "time") and m.shape == z1.shape + (len(time),)
    np.testing.assert_array_equal(m.coords["lat"].values, lat)
    np.testing.assert_array_equal(m.coords["lon"].values, lon)
    np.testing.assert_array_equal(m.coords["time"].values, time)
    assert list(m.doy[5:9]) == [365, 366, 1, 2]
    with pytest.raises(ValueError):
        get_daily_growing_season_mask(lat, lon, np.arange(4.0), ds)


def test_argument_errors_are_raised_before_any_device_work():
    import pandas as pd
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import minixr
    ds, z1, z2, lat, lon = growing_days()
    sw = pkg.season_windows(ds)
    time = np.arange("2001-01-01", "2001-01-04", dtype="datetime64[D]")
    field = minixr.Dataset({"tas": (("time", "lat", "lon"), np.zeros((3, len(lat), len(lon)), dtype=np.float32))},
                           coords={"time": time, "lat": lat, "lon": lon})
    df = pd.DataFrame({"lat": lat[:1], "lon": lon[:1], "areawt": [1.0], "popwt": [1.0], "reg": [0]})
    with pytest.raises(ValueError, match="period"):
        pkg.tas_poly_aggregate(field, [1], "popwt", "reg", df, season=sw)
    with pytest.raises(ValueError, match="_route"):
        pkg.tas_poly_aggregate(field, [1], "popwt", "reg", df, period="year", season=sw, _route="reduce_first")
    with pytest.raises(ValueError, match="_route"):
        pkg.weighted_aggregate_grid_to_regions_periods(field, "tas", "popwt", "reg", df, season=sw, _route="reduce_first")
    with pytest.raises(ValueError, match="_route"):
        pkg.weighted_aggregate_grid_to_regions_periods(field, "tas", "popwt", "reg", df, season=sw, _route="aggregate_first")
