"""Drop-in for the grid-level polynomial transform in front of the aggregation path
(SURVEY.md section 8f-3), fused into the aggregation kernels.

Reference (read as text): climate_toolbox/transformations/transformations.py
  tas_poly(ds, power, varname)   :160-208   (tas - 273.15) ** power, leap days removed, time -> YYYYDDD
  snyder_edd(tasmin, tasmax, e)  :7-93      Snyder exceedance degree days (nested xr.where, :75-87)
  snyder_gdd(tasmin, tasmax, lo, hi) :96-144   EDD(lo) - EDD(hi)
  validate_edd_snyder_agriculture(ds, thresholds) :150-157   24,378 hierid regions, every threshold in refTemp
  ordinal(n)                     :211-214
  climate_toolbox/utils/utils.py:74-77   remove_leap_days
  climate_toolbox/utils/utils.py:10-20   convert_kelvin_to_celsius

The reference evaluates the power on the whole grid on the host and hands the new grid to the
aggregation.  Here ``tas_poly`` returns a dataset whose variable still points at the Kelvin
buffer and carries ``(offset, power)``; ``weighted_aggregate_grid_to_regions`` evaluates the
transform on the GPU while the data is loaded (``wagg_apply_poly_*``), so the transformed grid is
never written anywhere.  ``tas_poly_aggregate`` does several powers in ONE pass over the data.
"""
from __future__ import annotations

import numpy as np

from . import minixr
from . import aggregations as _agg

__all__ = ["tas_poly", "tas_poly_aggregate", "snyder_edd", "snyder_gdd", "snyder_edd_aggregate", "snyder_exposure_aggregate",
           "tas_bins_aggregate",
           "tas_hinge_aggregate", "tas_rcspline_aggregate", "tas_spell_aggregate", "tas_rolling_aggregate",
           "tas_quantile_aggregate", "tas_relative_spell_aggregate",
           "validate_edd_snyder_agriculture", "ordinal", "remove_leap_days", "convert_kelvin_to_celsius"]

KELVIN = 273.15


def ordinal(n):
    """1 -> "1st", 2 -> "2nd", 3 -> "3rd", 4 -> "4th", 11 -> "11th", 22 -> "22nd" ...: the wording of the power in tas_poly's
    description attribute (same outputs as the reference's helper, transformations.py:211-214)."""
    n = int(n)
    last_two, last = n % 100, n % 10
    if 11 <= last_two <= 13 or last in (0, 4, 5, 6, 7, 8, 9):
        suffix = "th"
    else:
        suffix = {1: "st", 2: "nd", 3: "rd"}[last]
    return str(n) + suffix


def _month_day(time_values):
    t = np.asarray(time_values).astype("datetime64[D]")
    months = t.astype("datetime64[M]")
    month = months.astype(int) % 12 + 1
    day = (t - months.astype("datetime64[D]")).astype(int) + 1
    year = t.astype("datetime64[Y]").astype(int) + 1970
    return year, month, day


def remove_leap_days(ds):
    """Drop every 29 February along ``time`` (utils.py:74-77).  A dataset without one is returned as
    it is (no copy)."""
    _, month, day = _month_day(ds.coords["time"].values)
    keep = ~((month == 2) & (day == 29))
    if keep.all():
        return ds
    out = minixr.Dataset()
    for k, c in ds.coords.items():
        out.coords[k] = minixr.DataArray(np.asarray(c.values)[keep], c.dims) if c.dims == ("time",) else c
    for k, v in ds.data_vars.items():
        if "time" in v.dims:
            ax = v.dims.index("time")
            raw = _compress(v._values, keep, ax)
            if isinstance(v, minixr.LazyArray):            # keeps lon order, transform, degree-day partner, attrs
                edd_raw = None if v._edd is None else _compress(v._edd[0], keep, ax)
                out.data_vars[k] = v._replace(raw=raw, edd_raw=edd_raw, name=k)
            else:
                out.data_vars[k] = minixr.DataArray(raw, v.dims, name=k)
                out.data_vars[k].attrs = dict(getattr(v, "attrs", {}))
        else:
            out.data_vars[k] = v
    return out


def _compress(buf, keep, axis):
    if type(buf).__module__.startswith("torch"):          # device-resident buffer: wagg_take_axis
        from . import engine
        return engine.take_axis(buf, axis, np.flatnonzero(keep))
    return np.compress(keep, np.asarray(buf), axis=axis)


def convert_kelvin_to_celsius(df, temp_name):
    """Convert Kelvin to Celsius (utils.py:10-20) -- lazily: the variable keeps its Kelvin buffer
    and carries the offset, which the aggregation applies while loading."""
    v = df[temp_name]
    if getattr(v, "_xform", None) is not None or getattr(v, "_edd", None) is not None:
        raise ValueError("%r already carries a lazy transform" % (temp_name,))
    attrs = dict(getattr(v, "attrs", {}))
    attrs.update({"units": "C", "valid_min": -108.78788, "valid_max": 62.02828})
    df.data_vars[temp_name] = minixr.LazyArray(v._values, v.dims, lon_perm=getattr(v, "_lon_perm", None),
                                               xform=(-KELVIN, 1), name=temp_name, attrs=attrs)
    return df


def _day_index(ds):
    """transformations.py:191-199: ``time`` -> YYYYDDD integers (at most 365 days per call)."""
    ntime = len(ds.coords["time"].values)
    if ntime > 365:
        raise ValueError
    year, _, _ = _month_day(ds.coords["time"].values)
    return year * 1000 + np.arange(1, ntime + 1)


def _describe(power):
    raised = "" if power == 1 else " raised to the {powername} power".format(powername=ordinal(power))
    return ("Daily average temperature (degrees C){raised}\n\n"
            "            Leap years are removed before counting days (uses a 365 day\n"
            "            calendar).").format(raised=raised).strip()


def tas_poly(ds, power, varname):
    """Drop-in for transformations.py:160-208: ``(tas - 273.15) ** power`` as variable ``varname``,
    29 February dropped, ``time`` relabelled to YYYYDDD integers (at most 365 days per call).

    The returned variable is lazy (see the module docstring); ``.values`` evaluates it on demand.
    """
    if int(power) != power or power < 1:
        raise ValueError("power must be a positive integer, got %r" % (power,))
    power = int(power)
    description = _describe(power)
    ds = remove_leap_days(ds)
    tas = ds["tas"]
    if getattr(tas, "_xform", None) is not None:
        raise ValueError("'tas' already carries a lazy transform")
    day = _day_index(ds)
    ds1 = minixr.Dataset()
    for k, c in ds.coords.items():
        ds1.coords[k] = minixr.DataArray(day, ("time",)) if k == "time" else c
    attrs = {"units": "C^{}".format(power) if power > 1 else "C", "long_title": description.splitlines()[0],
             "description": description, "variable": varname}
    ds1.data_vars[varname] = minixr.LazyArray(tas._values, tas.dims, lon_perm=getattr(tas, "_lon_perm", None),
                                              xform=(-KELVIN, power), name=varname, attrs=attrs)
    return ds1


def tas_poly_aggregate(ds, powers, aggwt, agglev, weights, varnames=None, backup_aggwt="areawt", period=None, _route=None,
                       season=None, cells="all"):
    """``tas_poly`` for several powers followed by ``weighted_aggregate_grid_to_regions`` of each --
    as ONE pass over the temperature field (powers 1..4 of fp32 (time, lat, lon) data share a single
    read of the grid from HBM).  ``varnames`` defaults to ``tas-poly-<p>``.  Returns one Dataset
    with a variable per power, dims/coords as the reference's aggregation gives them.  ``period`` ("year", "month" or
    a label per remaining day; None: daily results as ever): every power summed over each period's days on the device, ``time``
    replaced by ``period`` (:func:`climate_toolbox_amd.periods.weighted_aggregate_grid_to_regions_periods`).  ``season`` (a
    growing-season mask, seasons.py; needs ``period``): only a cell's in-season days count, the days being those of the
    365-day calendar left after the leap-day drop.  ``cells`` ("all" | "referenced"; needs ``period``): as for
    :func:`climate_toolbox_amd.periods.weighted_aggregate_grid_to_regions_periods` -- "referenced" sums only the quads the
    table references."""
    if season is not None and period is None:
        raise ValueError("season= needs period=: a growing-season total is a sum over days")
    if season is not None and _route is not None:
        raise ValueError("_route cannot be combined with season=: season totals always sum the field first")
    from .periods import _check_cells
    _check_cells(cells, _route)
    if cells == "referenced" and period is None:
        raise ValueError("cells='referenced' needs period=: it sums the field over each period first")
    powers = [int(p) for p in powers]
    if not powers or min(powers) < 1 or len(set(powers)) != len(powers):
        raise ValueError("powers must be distinct positive integers, got %r" % (powers,))
    if varnames is None:
        varnames = ["tas-poly-%d" % p for p in powers]
    if len(varnames) != len(powers):
        raise ValueError("one variable name per power")
    if isinstance(weights, str):
        weights = _agg.prepare_spatial_weights_data(weights)
    ds = remove_leap_days(ds)
    day = _day_index(ds)
    ds = minixr.Dataset({"tas": ds["tas"]}, coords={k: (minixr.DataArray(day, ("time",)) if k == "time" else c)
                                                  for k, c in ds.coords.items()})
    grid = None if season is None else (np.asarray(ds.coords["lat"].values), np.asarray(ds.coords["lon"].values))
    re = _agg._reindex_spatial_data_to_regions(ds, weights)
    if period is not None:
        from . import periods
        return periods._aggregate_periods(re, varnames, aggwt, agglev, weights, backup_aggwt, period, day, powers=powers,
                                          offset=-KELVIN, route=_route, season=season, grid=grid, cells=cells)
    res, rdims, coords, was_xr = _agg._aggregate_core(re, "tas", aggwt, agglev, weights, backup_aggwt,
                                                      powers=powers, offset=-KELVIN)
    return _agg._as_dataset(dict(zip(varnames, res)), rdims, coords, was_xr)


def _units(arr):
    return getattr(arr, "attrs", {}).get("units")


def _degree_days(tasmin, tasmax, terms, units):
    for a in (tasmin, tasmax):
        if getattr(a, "_edd", None) is not None or (getattr(a, "_xform", None) is not None and a._xform[1] != 1):
            raise ValueError("degree days need plain (or Kelvin-shifted) temperature fields")
    off_lo = tasmin._xform[0] if getattr(tasmin, "_xform", None) is not None else 0.0
    off_hi = tasmax._xform[0] if getattr(tasmax, "_xform", None) is not None else 0.0
    if off_lo != off_hi:
        raise ValueError("tasmin and tasmax carry different offsets")
    lo, hi = tasmin._values, tasmax._values
    if tuple(tasmin.dims) != tuple(tasmax.dims) or lo.shape != hi.shape or lo.dtype != hi.dtype:
        raise ValueError("tasmin and tasmax must have the same dims, shape and dtype")
    plo, phi = getattr(tasmin, "_lon_perm", None), getattr(tasmax, "_lon_perm", None)
    if (plo is None) != (phi is None) or (plo is not None and not np.array_equal(plo, phi)):
        raise ValueError("tasmin and tasmax must share their longitude order")
    # check to make sure tasmax > tasmin everywhere (transformations.py:62), on the device
    # (wagg_any_less_*).  Host buffers are uploaded for this check and again by the aggregation:
    # hand device tensors in to avoid both copies.
    from . import engine
    engine.require_gpu()
    bad = engine.any_less(engine.to_device(hi), engine.to_device(lo))
    assert not bad, "values encountered where tasmin > tasmax"
    return minixr.LazyArray(lo, tasmin.dims, lon_perm=plo, edd=(hi, off_lo, terms), name=tasmin.name,
                            attrs={"units": units})


def snyder_edd(tasmin, tasmax, threshold):
    """Drop-in for transformations.py:7-93: degree days above ``threshold`` of the sinusoid through
    the daily (tasmin, tasmax) pair -- both DataArrays of one Dataset, in degrees C like the
    threshold.  The result is a lazy variable: assign it to a Dataset and hand that to
    ``weighted_aggregate_grid_to_regions`` -- the degree days are evaluated on the GPU while both
    fields are loaded (``wagg_apply_edd_*``); ``.values`` materialises the grid on demand.
    """
    assert _units(tasmin) == _units(tasmax)                    # :56, same units on both fields
    return _degree_days(tasmin, tasmax, [(1.0, float(threshold))],
                        "degreedays_{}{}".format(threshold, _units(tasmax)))


def snyder_gdd(tasmin, tasmax, threshold_low, threshold_high):
    """Drop-in for transformations.py:96-144: EDD(threshold_low) - EDD(threshold_high).  Lazy like
    :func:`snyder_edd`; the aggregation of the difference is the difference of the two aggregations.
    """
    assert _units(tasmin) == _units(tasmax)                    # :133
    return _degree_days(tasmin, tasmax, [(1.0, float(threshold_low)), (-1.0, float(threshold_high))],
                        "degreedays_{}-{}{}".format(threshold_low, threshold_high, _units(tasmax)))


def _ladder_thresholds(thresholds):
    """``thresholds`` as a float64 vector, in the caller's order: non-empty, finite, distinct -- else ValueError"""
    try:
        thr = np.asarray(list(thresholds), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("thresholds must be a sequence of numbers, got %r" % (thresholds,)) from None
    if thr.ndim != 1 or len(thr) == 0 or not np.isfinite(thr).all() or len(np.unique(thr)) != len(thr):
        raise ValueError("thresholds must be a non-empty sequence of distinct finite numbers, got %r" % (thresholds,))
    return thr


def _period_lists(ds, period, season):
    """``(time_values, labels, grid, lists)`` of a period call on ``ds`` (which has a ``time`` coordinate): the period labels,
    the dataset's own lat / lon labels for a ``season=`` call (else None), and ``lists(device)`` -- the periods' row lists as
    ``engine.period_lists`` uploads them, once per device"""
    from . import periods
    time_values = np.asarray(ds.coords["time"].values)
    labels, row_begin, rows = periods.period_rows(time_values, period)
    grid = None if season is None else (np.asarray(ds.coords["lat"].values), np.asarray(ds.coords["lon"].values))
    cache = {}

    def lists(device):
        if str(device) not in cache:
            cache[str(device)] = periods._engine.period_lists(row_begin, rows, len(time_values), device=device)
        return cache[str(device)]

    lists.row_begin = np.asarray(row_begin, dtype=np.int64)          # (the host offsets: a caller that needs the lists' lengths)
    return time_values, labels, grid, lists


def _time_as_period(rdims, coords, labels):
    """the dims and coords of a sum-first result with ``time`` replaced by ``period`` = ``labels``"""
    return tuple("period" if d == "time" else d for d in rdims), dict({k: v for k, v in coords.items() if k != "time"}, period=labels)


def snyder_edd_aggregate(ds, thresholds, aggwt, agglev, weights, tasmin="tasmin", tasmax="tasmax", varname="edd",
                         backup_aggwt="areawt", period=None, season=None, cells="all"):
    """Snyder degree days at EVERY threshold of a ladder, aggregated to regions: the reference's agricultural product (what
    ``validate_edd_snyder_agriculture`` accepts), in one call -- ``snyder_edd`` of ``ds[tasmin]`` / ``ds[tasmax]`` (degrees C, or
    Kelvin fields shifted by ``convert_kelvin_to_celsius``; same checks: equal units, tasmin <= tasmax everywhere) for every
    ``thresholds[k]`` (a non-empty sequence of distinct finite numbers, else ValueError), then the aggregation of each.

    Returns one Dataset with the variable ``varname`` of dims ``("refTemp", "period" | "time", agglev)`` (the last two in the
    order the single call gives them), the coordinate ``refTemp`` = the thresholds as float64 in the caller's order, and
    ``attrs["units"] = "degreedays_" + units``; period and region coordinates as
    :func:`~climate_toolbox_amd.periods.weighted_aggregate_grid_to_regions_periods` gives them; ``results_on_device()`` is honoured.

    period   "year", "month" or a label per day, as there: both fields are summed per period and threshold first, in ONE launch
             per 64 thresholds (``wagg_edd_ladder_reduce_*``), and one apply contracts the n_thr x P rows -- whatever the plan;
             a (lat, lon, time) field is transposed on the device, a host-resident one uploaded whole.  A counted +-inf raises
             ValueError.  None: daily results, from the fused daily apply in groups of up to four thresholds.
    season   a growing-season mask (seasons.py; needs ``period``): only a cell's in-season days count.
    cells    "all" or "referenced" (needs ``period``): as for ``weighted_aggregate_grid_to_regions_periods`` -- "referenced" packs
             both fields to the quads the table references, evaluates every threshold on those cells only and contracts through
             the plan's quads-only cell table; a +-inf in a quad no table row reads is not seen."""
    thr = _ladder_thresholds(thresholds)
    if season is not None and period is None:
        raise ValueError("season= needs period=: a growing-season total is a sum over days")
    from .periods import _check_cells
    _check_cells(cells)
    if cells == "referenced" and period is None:
        raise ValueError("cells='referenced' needs period=: it sums the field over each period first")
    if isinstance(weights, str):
        weights = _agg.prepare_spatial_weights_data(weights)
    lo, hi = ds[tasmin], ds[tasmax]
    assert _units(lo) == _units(hi)
    units = "degreedays_{}".format(_units(hi))

    base = _degree_days(lo, hi, [(1.0, float(thr[0]))], units)       # (the checks of snyder_edd, once for the whole ladder)

    def reindexed(lo_buf, hi_buf):
        var = minixr.LazyArray(lo_buf, base.dims, lon_perm=base._lon_perm, edd=(hi_buf, base._edd[1], base._edd[2]), name=varname)
        return _agg._reindex_spatial_data_to_regions(minixr.Dataset({varname: var}, coords=dict(ds.coords)), weights)

    if period is not None:
        from . import seasons
        if "time" not in ds.coords:
            raise ValueError("the dataset has no 'time' coordinate to form periods from")
        time_values, labels, grid, lists = _period_lists(ds, period, season)
        res, rdims, coords, was_xr = seasons._ladder_totals(reindexed(base._values, base._edd[0]), varname, aggwt, agglev, weights,
                                                            backup_aggwt, lists, len(labels), thr, season, grid, time_values, cells=cells)
        rdims, coords = _time_as_period(rdims, coords, labels)
    else:
        # daily results: the fused daily apply takes four thresholds a pass.  The table is joined to the grid once and a
        # host-resident pair of fields uploaded once; every pass then reads the same two device buffers.
        from . import engine
        from ._layout import _is_device_tensor
        from ._pinned import _to_host
        on_host = not _is_device_tensor(base._values)
        re = reindexed(engine.to_device(base._values), engine.to_device(base._edd[0]))
        hi_dev, off = re._edds[varname][0], re._edds[varname][1]
        planes = []
        for k0 in range(0, len(thr), 4):
            re._edds[varname] = (hi_dev, off, [(1.0, float(e)) for e in thr[k0:k0 + 4]])
            got, rdims, coords, was_xr = _agg._aggregate_core(re, varname, aggwt, agglev, weights, backup_aggwt, edd_planes=True)
            planes.extend(got)
        if _is_device_tensor(planes[0]):                             # (results_on_device(): of a device-resident field only)
            res = _to_host(engine.require_gpu().stack(planes)) if on_host else engine.require_gpu().stack(planes)
        else:
            res = np.stack(planes)
    out = _agg._as_dataset({varname: res}, ("refTemp",) + tuple(rdims), dict(coords, refTemp=thr), was_xr)
    out[varname].attrs["units"] = units
    return out


def snyder_exposure_aggregate(ds, edges, aggwt, agglev, weights, tasmin="tasmin", tasmax="tasmax", varname="exposure",
                              backup_aggwt="areawt", period="year", season=None, cells="all"):
    """The time a day's sinusoidal temperature curve spends in each bin ``[edges[k], edges[k + 1])`` -- the Schlenker-Roberts
    exposure bins -- summed per period (and growing season) and aggregated to regions.  The curve is the single sine through
    ``ds[tasmin]`` / ``ds[tasmax]`` that :func:`snyder_edd` integrates (same checks: equal units, tasmin <= tasmax everywhere;
    degrees C, or Kelvin fields shifted by ``convert_kelvin_to_celsius``), and the fraction of a day above ``e`` is the
    derivative of the degree-day ladder, ``A(e) = -d EDD / de``; bin ``k`` of a day is ``A(edges[k]) - A(edges[k + 1])``.
    Where :func:`tas_bins_aggregate` puts a 22-38 C day wholly into the bin of its mean, this call spreads it over every bin
    its curve passes through.  One launch per 64 bins (``wagg_exposure_reduce_*``) instead of two passes over the grid per edge.

    edges    as for :func:`tas_bins_aggregate`: at least two strictly ascending numbers, ``-inf`` allowed first and ``+inf``
             last, else ValueError; converted to the element type.  A day with NaN in either field is in no bin; a counted
             +-inf raises ValueError.
    period   "year", "month" or a label per day; required (None is ValueError: an exposure total is a sum over days).
    season, cells   exactly as in :func:`snyder_edd_aggregate`; "referenced" packs both fields.

    Returns one Dataset with the variable ``varname`` of dims ``("bin", "period", agglev)`` (the last two in the order the
    period call gives them), the coordinate ``bin`` = the lower edges as float64, ``attrs["units"] = "days"`` and
    ``attrs["bin_edges"]`` as :func:`tas_bins_aggregate` writes them; ``results_on_device()`` is honoured."""
    e = _bin_edges(edges)
    if period is None:
        raise ValueError("snyder_exposure_aggregate needs period=: an exposure total is a sum over days"
                         + ("" if season is None else " (season= needs period=)"))
    from .periods import _check_cells
    _check_cells(cells)
    if isinstance(weights, str):
        weights = _agg.prepare_spatial_weights_data(weights)
    lo, hi = ds[tasmin], ds[tasmax]
    assert _units(lo) == _units(hi)
    base = _degree_days(lo, hi, [(1.0, 0.0)], "days")                # (the checks of snyder_edd; the terms are not used)
    if "time" not in ds.coords:
        raise ValueError("the dataset has no 'time' coordinate to form periods from")
    var = minixr.LazyArray(base._values, base.dims, lon_perm=base._lon_perm, edd=base._edd, name=varname)
    re = _agg._reindex_spatial_data_to_regions(minixr.Dataset({varname: var}, coords=dict(ds.coords)), weights)
    from . import seasons
    time_values, labels, grid, lists = _period_lists(ds, period, season)
    res, rdims, coords, was_xr = seasons._exposure_totals(re, varname, aggwt, agglev, weights, backup_aggwt, lists, len(labels), e, season,
                                                          grid, time_values, cells=cells)
    rdims, coords = _time_as_period(rdims, coords, labels)
    out = _agg._as_dataset({varname: res}, ("bin",) + tuple(rdims), dict(coords, bin=e[:-1].copy()), was_xr)
    out[varname].attrs["units"] = "days"
    out[varname].attrs["bin_edges"] = ", ".join(repr(float(x)) for x in e)
    return out


def _period_setup(name, what, ds, tas, weights, period, season, cells, leap_days):
    """What :func:`tas_bins_aggregate` and the hinge calls do alike behind the checks of their own parameter list, in this order:
    the period / cells / leap_days checks (``name``: the public call, ``what``: "a bin count" / "a hinge total", for the
    messages), weights read from a path, the ``time`` coordinate, ``remove_leap_days``, the rule that ``ds[tas]`` is a plain or
    Kelvin-shifted temperature variable, the period lists, and the variable joined to the table.  Returns ``(reindexed dataset,
    variable, weights, time_values, labels, grid, lists)``."""
    if period is None:
        raise ValueError("%s needs period=: %s is a sum over days" % (name, what) + ("" if season is None else " (season= needs period=)"))
    from .periods import _check_cells
    _check_cells(cells)
    if leap_days not in ("keep", "drop"):
        raise ValueError("leap_days must be 'keep' or 'drop', got %r" % (leap_days,))
    if isinstance(weights, str):
        weights = _agg.prepare_spatial_weights_data(weights)
    if "time" not in ds.coords:
        raise ValueError("the dataset has no 'time' coordinate to form periods from")
    if leap_days == "drop":
        ds = remove_leap_days(ds)
    var = ds[tas]
    xform = getattr(var, "_xform", None)
    if getattr(var, "_edd", None) is not None or (xform is not None and xform[1] != 1):
        raise ValueError("%s needs a plain (or Kelvin-shifted) temperature variable, got %r" % (what, tas))
    time_values, labels, grid, lists = _period_lists(ds, period, season)
    re = _agg._reindex_spatial_data_to_regions(minixr.Dataset({tas: var}, coords=dict(ds.coords)), weights)
    return re, var, weights, time_values, labels, grid, lists


def _bin_edges(edges):
    """``edges`` as a float64 vector: at least two numbers, strictly ascending, no NaN (infinite ends allowed) -- else ValueError"""
    try:
        e = np.asarray(list(edges), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("edges must be a sequence of numbers, got %r" % (edges,)) from None
    if e.ndim != 1 or len(e) < 2 or np.isnan(e).any() or not (e[1:] > e[:-1]).all():
        raise ValueError("edges must be at least two strictly ascending numbers (-inf / +inf allowed at the ends), got %r" % (edges,))
    return e


def tas_bins_aggregate(ds, edges, aggwt, agglev, weights, tas="tas", varname="tas-bins", backup_aggwt="areawt", period="year",
                       season=None, cells="all", leap_days="keep"):
    """The days a cell's daily mean temperature spends in each bin ``[edges[k], edges[k + 1])``, summed per period (and growing
    season) and aggregated to regions: the third temperature statistic of climate-impact regressions beside the polynomials
    (:func:`tas_poly_aggregate`) and the degree days (:func:`snyder_edd_aggregate`), counted on the device in ONE pass per 64
    bins (``wagg_bin_days_reduce_*``) instead of one masked grid per bin.

    edges    at least two strictly ascending numbers, ``-inf`` allowed first and ``+inf`` last (open end bins), else ValueError;
             in degrees C when ``ds[tas]`` carries the Kelvin shift of ``convert_kelvin_to_celsius``, otherwise in the field's own
             units.  A value equal to an edge lands in the upper bin.  The comparison is exact: the raw value is compared
             against ``edges[k] - offset`` rounded UP to the element type, so an fp32 Kelvin field is binned as its exact
             values would be in fp64 (``engine.bin_thresholds``).  NaN is in no bin; a counted +-inf raises ValueError.
    tas      the variable: a plain temperature field or a Kelvin-shifted one; a power (``tas_poly``) or a degree-day variable
             is ValueError.
    period   "year", "month" or a label per day, as for
             :func:`~climate_toolbox_amd.periods.weighted_aggregate_grid_to_regions_periods`; required (None is ValueError: a
             bin count is a sum over days).
    season, cells   exactly as in :func:`snyder_edd_aggregate`.
    leap_days   "keep" (the default) or "drop": ``remove_leap_days`` first, as ``tas_poly`` does.

    Returns one Dataset with the variable ``varname`` of dims ``("bin", "period", agglev)`` (the last two in the order the
    period call gives them), the coordinate ``bin`` = the lower edges as float64, ``attrs["units"] = "days"`` and
    ``attrs["bin_edges"]`` = the edges as one string (``", ".join(repr(float(e)) ...)``); ``results_on_device()`` is honoured;
    a (lat, lon, time) field is transposed on the device, a host-resident one uploaded whole (packed for "referenced")."""
    e = _bin_edges(edges)
    re, _, weights, time_values, labels, grid, lists = _period_setup("tas_bins_aggregate", "a bin count", ds, tas, weights, period, season,
                                                                     cells, leap_days)
    from . import seasons
    res, rdims, coords, was_xr = seasons._bin_totals(re, tas, aggwt, agglev, weights, backup_aggwt, lists, len(labels), e, season, grid,
                                                     time_values, cells=cells)
    rdims, coords = _time_as_period(rdims, coords, labels)
    out = _agg._as_dataset({varname: res}, ("bin",) + tuple(rdims), dict(coords, bin=e[:-1].copy()), was_xr)
    out[varname].attrs["units"] = "days"
    out[varname].attrs["bin_edges"] = ", ".join(repr(float(x)) for x in e)
    return out


def _check_side(side):
    if side not in ("above", "below"):
        raise ValueError("side must be 'above' or 'below', got %r" % (side,))


def _hinge_call(name, ds, knots, tail, power, side, aggwt, agglev, weights, tas, backup_aggwt, period, season, cells, leap_days):
    """what :func:`tas_hinge_aggregate` and :func:`tas_rcspline_aggregate` do alike behind their own checks of the knots: the
    remaining argument checks, the period lists and ``seasons._hinge_totals``.  Returns ``(stack, rdims, coords, was_xarray,
    units)`` with "time" already renamed to "period"."""
    if power not in (1, 2, 3):
        raise ValueError("power must be 1, 2 or 3, got %r" % (power,))
    _check_side(side)
    re, var, weights, time_values, labels, grid, lists = _period_setup(name, "a hinge total", ds, tas, weights, period, season, cells,
                                                                       leap_days)
    from . import seasons
    res, rdims, coords, was_xr = seasons._hinge_totals(re, tas, aggwt, agglev, weights, backup_aggwt, lists, len(labels), knots, power,
                                                       side, tail, season, grid, time_values, cells=cells)
    rdims, coords = _time_as_period(rdims, coords, labels)
    return res, rdims, coords, was_xr, _units(var)


def tas_hinge_aggregate(ds, knots, aggwt, agglev, weights, power=1, side="above", tas="tas", varname="tas-hinge", backup_aggwt="areawt",
                        period="year", season=None, cells="all", leap_days="keep"):
    """Truncated powers of a cell's daily temperature about every knot of a list, ``max(+-(tas - k), 0) ** power``, summed per
    period (and growing season) and aggregated to regions: the fourth temperature statistic of climate-impact regressions
    beside the polynomials (:func:`tas_poly_aggregate`), the Snyder degree days (:func:`snyder_edd_aggregate`) and the bins
    (:func:`tas_bins_aggregate`), evaluated on the device in ONE pass per 64 knots (``wagg_hinge_reduce_*``) instead of one
    clamped grid per knot.  With ``power=1`` on the daily mean these are the plain degree days of the energy sector: cooling
    degree days are side ``"above"`` (``max(tas - k, 0)``), heating degree days are side ``"below"`` (``max(k - tas, 0)``);
    ``power=1`` at several knots is a linear spline; ``power=3`` gives the truncated cubes of a cubic spline
    (:func:`tas_rcspline_aggregate` combines them into the restricted one).

    knots    a non-empty sequence of distinct finite numbers, in any order, else ValueError; in degrees C when ``ds[tas]``
             carries the Kelvin shift of ``convert_kelvin_to_celsius``, otherwise in the field's own units.  More than 64 knots
             go in several launches.  The difference ``d = (tas + offset) - k`` is formed in the element type, so an fp32
             Kelvin field carries up to one ulp of the Kelvin value (3e-5 K) into a hinge -- unlike the bins' exact
             comparison; powers are products in the element type, sums over days are fp64.  NaN counts 0; a counted +-inf
             raises ValueError.
    power    1, 2 or 3;  side: "above" or "below" -- else ValueError.
    tas      the variable: a plain temperature field or a Kelvin-shifted one; a power (``tas_poly``) or a degree-day variable
             is ValueError.
    period   "year", "month" or a label per day, as for
             :func:`~climate_toolbox_amd.periods.weighted_aggregate_grid_to_regions_periods`; required (None is ValueError).
    season, cells, leap_days   exactly as in :func:`tas_bins_aggregate`.

    Returns one Dataset with the variable ``varname`` of dims ``("knot", "period", agglev)`` (the last two in the order the
    period call gives them), the coordinate ``knot`` = the knots as float64 in the caller's order, ``attrs["units"]`` =
    ``"degreedays_" + units`` for ``power == 1`` and ``units + "^" + str(power)`` otherwise, and ``attrs["side"]``;
    ``results_on_device()`` is honoured; a (lat, lon, time) field is transposed on the device, a host-resident one uploaded
    whole (packed for "referenced")."""
    k = _ladder_thresholds(knots)
    res, rdims, coords, was_xr, units = _hinge_call("tas_hinge_aggregate", ds, k, None, power, side, aggwt, agglev, weights, tas,
                                                    backup_aggwt, period, season, cells, leap_days)
    out = _agg._as_dataset({varname: res}, ("knot",) + tuple(rdims), dict(coords, knot=k), was_xr)
    out[varname].attrs["units"] = "degreedays_{}".format(units) if power == 1 else "{}^{}".format(units, power)
    out[varname].attrs["side"] = side
    return out


def _rcspline_knots(knots):
    """``knots`` as a float64 vector: 3 to 66 strictly ascending finite numbers -- else ValueError"""
    try:
        t = np.asarray(list(knots), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("knots must be a sequence of numbers, got %r" % (knots,)) from None
    if t.ndim != 1 or not 3 <= len(t) <= 66 or not np.isfinite(t).all() or not (t[1:] > t[:-1]).all():
        raise ValueError("knots must be 3 to 66 strictly ascending finite numbers, got %r" % (knots,))
    return t


def tas_rcspline_aggregate(ds, knots, aggwt, agglev, weights, tas="tas", varname="tas-rcspline", normalize=False, backup_aggwt="areawt",
                           period="year", season=None, cells="all", leap_days="keep"):
    """The nonlinear terms of a restricted (natural) cubic spline of a cell's daily temperature, summed per period (and growing
    season) and aggregated to regions -- the usual alternative to the fourth-order polynomial.  For knots ``t_1 < ... < t_K``
    the ``K - 2`` terms are, with ``u+ = max(u, 0)``,

        term_j = (x - t_j)+^3 - (x - t_{K-1})+^3 * (t_K - t_j) / (t_K - t_{K-1}) + (x - t_K)+^3 * (t_{K-1} - t_j) / (t_K - t_{K-1})

    for ``j = 1 .. K - 2``: each is 0 below ``t_1`` and linear beyond ``t_K``.  ONE kernel call serves all terms: the cubes at
    the last two knots are summed beside those of every ``t_j`` and combined with them in fp64 before the cast
    (``wagg_hinge_reduce_*`` with its tail), so the cancellation beyond the last knot never happens in fp32.  The spline's
    linear term is :func:`tas_poly` with power 1 (``tas_poly_aggregate(..., powers=[1])``): it is not repeated here.

    knots      3 to 66 strictly ascending finite numbers, else ValueError; units as for :func:`tas_hinge_aggregate`.
    normalize  True: every term is divided by ``(t_K - t_1) ** 2`` (Harrell's scaling, which puts the terms on the scale of x; applied
               to the results as one multiplication by the reciprocal).
    everything else as for :func:`tas_hinge_aggregate` (the differences are formed in the element type there as here).

    Returns one Dataset with the variable ``varname`` of dims ``("term", "period", agglev)``, the coordinate ``term`` =
    ``knots[:-2]`` as float64, ``attrs["units"] = units + "^3"`` and ``attrs["knots"]`` = the knots as one string
    (``", ".join(repr(float(t)) ...)``)."""
    t = _rcspline_knots(knots)
    span = t[-1] - t[-2]
    ca, cb = -(t[-1] - t[:-2]) / span, (t[-2] - t[:-2]) / span
    res, rdims, coords, was_xr, units = _hinge_call("tas_rcspline_aggregate", ds, t[:-2], (t[-2:].copy(), ca, cb), 3, "above", aggwt,
                                                    agglev, weights, tas, backup_aggwt, period, season, cells, leap_days)
    if normalize:                                                    # (one multiplication: the same bits from a host array and a device tensor)
        res = res * (1.0 / float((t[-1] - t[0]) ** 2))
    out = _agg._as_dataset({varname: res}, ("term",) + tuple(rdims), dict(coords, term=t[:-2].copy()), was_xr)
    out[varname].attrs["units"] = "{}^3".format(units)
    out[varname].attrs["knots"] = ", ".join(repr(float(x)) for x in t)
    return out


def _spell_thresholds(thresholds):
    """``thresholds`` as a float64 vector in the caller's order: at least one finite number (duplicates allowed) -- else ValueError"""
    try:
        t = np.asarray(list(thresholds), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("thresholds must be a sequence of numbers, got %r" % (thresholds,)) from None
    if t.ndim != 1 or len(t) < 1 or not np.isfinite(t).all():
        raise ValueError("thresholds must be a non-empty sequence of finite numbers, got %r" % (thresholds,))
    return t


def _spell_options(stat, side, min_length, stats, unset):
    """``stat`` (one of ``stats``), ``side`` and ``min_length`` of a public spell call, checked in that order -- else ValueError.
    The statistics of ``unset`` do not use ``min_length``: its default 3 counts as unset there, anything but that or 1 is
    ValueError.  Returns the ``min_length`` the device call gets."""
    if stat not in stats:
        raise ValueError("stat must be %s or %r, got %r" % (", ".join(repr(s) for s in stats[:-1]), stats[-1], stat))
    _check_side(side)
    if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)) or not 1 <= min_length <= 32767:
        raise ValueError("min_length must be an integer in 1..32767, got %r" % (min_length,))
    if stat in unset:
        if min_length not in (1, 3):
            raise ValueError("stat=%r does not use min_length (leave it out, or pass 1), got %r" % (stat, int(min_length)))
        return 1
    return int(min_length)


def _spell_attrs(attrs, stat, side, min_length, sum_units=None):
    """what the two public spell calls say of a result: units by statistic (``sum_units`` for the two sums; None: not said),
    ``min_length``, ``stat``, ``side``"""
    units = sum_units if stat in ("amount", "excess") else "1" if stat == "events" else "days"
    if units is not None:
        attrs["units"] = units
    attrs["min_length"] = min_length
    attrs["stat"] = stat
    attrs["side"] = side


def tas_spell_aggregate(ds, thresholds, aggwt, agglev, weights, min_length=3, stat="days", side="above", tas="tas", varname="tas-spell",
                        backup_aggwt="areawt", period="year", season=None, cells="all", leap_days="keep", span="period"):
    """Spell statistics of a cell's daily temperature -- runs of consecutive days past a threshold -- per period (and growing
    season), aggregated to regions: heat-wave and cold-spell days, the number of such events and the longest run (the ETCCDI /
    xclim spell indices; ``tas="tasmax"``, threshold 35 C, ``min_length=3`` is the usual heat wave).  The one temperature
    statistic here in which a day's contribution depends on its neighbours, counted on the device in ONE pass per 64 thresholds
    (``wagg_spell_reduce_*``) instead of a run-length scan and a masked grid per threshold.

    A day is hot for a threshold when ``tas >= threshold`` (``side="above"``) or ``tas < threshold`` (``"below"``); a run is a
    maximal stretch of hot, in-season, CONSECUTIVE days of one period.  A missing day, a day out of season and a NaN end a run,
    and so does the end of the period: RUNS ARE TRUNCATED AT PERIOD BOUNDARIES (a heat wave over New Year's Eve counts as one
    run in each of the two years; with ``period="month"`` every month starts anew; with labels that join the Januaries of
    several years, a run never reaches from one January into the next).  With ``leap_days="drop"`` 28 February and 1 March are consecutive.
    That is ``span="period"``, the default; ``span="record"`` (below) lets the runs continue across the boundaries.

    thresholds  a non-empty sequence of finite numbers in any order, duplicates allowed, else ValueError; in degrees C when
                ``ds[tas]`` carries the Kelvin shift of ``convert_kelvin_to_celsius``, otherwise in the field's own units.  More
                than 64 go in several launches.  The comparison is the bins' exact one: an fp32 Kelvin field is classified as
                its exact values would be in fp64 (``engine.bin_thresholds``).  NaN is never hot; a counted +-inf raises
                ValueError.
    min_length  an integer in 1..32767, else ValueError: the least length of a run that counts.
    stat        "days": the days that belong to runs of at least ``min_length``; "events": the number of such runs; "longest":
                the length of the longest run -- ``min_length`` is not used there, its default counts as unset, and any value
                other than 1 or the default is ValueError.
    side        "above" or "below", else ValueError.
    tas         the variable (``"tasmax"`` for heat waves): a plain temperature field or a Kelvin-shifted one; a power
                (``tas_poly``) or a degree-day variable is ValueError.
    period      "year", "month" or a label per day; required (None is ValueError).
    season, cells, leap_days   exactly as in :func:`tas_bins_aggregate`.
    span        "period" (runs truncated at period boundaries, as above) or "record", else ValueError.  ``span="record"``
                (``wagg_spell_span_*``) counts SPELLS THAT RUN ACROSS PERIOD BOUNDARIES.  The CHAIN is the concatenation
                of the periods' day lists in period order.  A day is hot as above; it JOINS the chain's day before when it is the
                next day of the record (under ``leap_days="drop"`` 31 December and 1 January of consecutive years join, as 28
                February and 1 March do), whether or not a period boundary or several empty periods lie between them; a RUN is
                a maximal stretch of hot, joined days of the chain; the RUNNING LENGTH ``r_i`` of a day is its position within
                its run, from 1, or 0 when cold, and is carried over boundaries; ``l`` is the run's WHOLE LENGTH.  With ``L =
                min_length``: "days" counts the hot days of the period whose run has ``l >= L`` -- every day in its own period,
                whether it counts being decided by the whole run; "events" counts the days of the period with ``r_i == L`` -- a
                run counts once, in the period in which it reaches ``min_length`` (``L = 1``: in which it starts); "longest"
                is the greatest ``r_i`` over the days of the period, 0 for an empty one -- a spell counts in a period for as
                long as it has lasted by then, reaching back to its start wherever that lies: a year wholly inside one dry
                spell reports at least its own length, a spell from 20 December to 10 January gives 12 and 22.  Where no run
                crosses a boundary the result is ``span="period"``'s.  ETCCDI's CDD, the longest dry spell, is
                ``tas="pr", thresholds=[1.0], stat="longest", side="below", span="record"`` for pr in mm/day, and CWD the
                same with ``side="above"``; both are defined on spells that run through New Year.  Joins are found only
                between neighbours in the chain, so the mode means something for periods whose lists follow each other in
                time: "year", "month", ascending labels.  With labels that pool the Januaries of all years nothing joins
                across the lists and the result equals ``span="period"``; that is not an error.  The per-cell-threshold call
                (:func:`tas_relative_spell_aggregate`) keeps truncating.

    The regional value is the weighted mean of the per-cell counts (for "longest": of the per-cell longest runs).  Returns one
    Dataset with the variable ``varname`` of dims ``("threshold", "period", agglev)`` (the last two in the order the period call
    gives them), the coordinate ``threshold`` = the thresholds as float64 in the caller's order, ``attrs["units"]`` = ``"days"``
    (days, longest) or ``"1"`` (events) and ``attrs["min_length"]`` (1 for "longest"), ``attrs["stat"]``, ``attrs["side"]``,
    ``attrs["span"]``; ``results_on_device()`` is honoured."""
    t = _spell_thresholds(thresholds)
    if span not in ("period", "record"):
        raise ValueError("span must be 'period' or 'record', got %r" % (span,))
    min_length = _spell_options(stat, side, min_length, ("days", "events", "longest"), ("longest",))
    re, _, weights, time_values, labels, grid, lists = _period_setup("tas_spell_aggregate", "a spell count", ds, tas, weights, period,
                                                                     season, cells, leap_days)
    from . import seasons
    res, rdims, coords, was_xr = seasons._spell_totals(re, tas, aggwt, agglev, weights, backup_aggwt, lists, len(labels), t, min_length,
                                                       stat, side, season, grid, time_values, cells=cells, span=span)
    rdims, coords = _time_as_period(rdims, coords, labels)
    out = _agg._as_dataset({varname: res}, ("threshold",) + tuple(rdims), dict(coords, threshold=t.copy()), was_xr)
    _spell_attrs(out[varname].attrs, stat, side, min_length)
    out[varname].attrs["span"] = span
    return out


def tas_relative_spell_aggregate(ds, thresholds, aggwt, agglev, weights, min_length=3, stat="days", side="above", tas="tas",
                                 varname="tas-relative-spell", backup_aggwt="areawt", period="year", planes=None, season=None,
                                 cells="all", leap_days="keep"):
    """:func:`tas_spell_aggregate` against thresholds that are each CELL'S OWN: days above the cell's 90th percentile of a
    baseline (TX90p / TN10p), warm-spell days in runs of at least 6 such days (WSDI / CSDI), heat-wave events above the local
    95th percentile, and with ``stat="amount"`` on precipitation the rain that falls on days above the cell's 95th wet-day
    percentile (R95pTOT).  Counted on the device in ONE pass per 64 levels (``wagg_cell_spells_*``), the thresholds read per
    cell, instead of a boolean grid, a run-length scan and a masked field per level.

    thresholds  a :class:`~climate_toolbox_amd.relative.CellThresholds`: what
                :func:`~climate_toolbox_amd.relative.cell_quantiles` returned for a baseline, or a caller's own field
                (``CellThresholds.from_array``).  Its grid is joined to the dataset's ``lat`` / ``lon`` by exact label equality
                (ValueError for a dataset cell it lacks) and its values are converted to the field's dtype once.  The comparison is
                :func:`tas_spell_aggregate`'s exact one, with the kernel's offset = the variable's Kelvin shift minus
                ``thresholds.shift``: exactly 0 when both come from the same Kelvin variable, so raw elements are compared with raw
                order statistics.  A cell whose threshold is NaN has NO VALUE there and enters the regional mean as a NaN of
                :func:`tas_quantile_aggregate` does.  More than 64 levels go in several launches.
    planes      which plane of ``thresholds`` a period reads.  None: there is one plane, or the plane labels equal the period
                labels one to one.  "month": a period labelled ``year * 100 + month`` reads the plane labelled ``month``.  A
                callable maps a period label to a plane label.  A period without a plane is ValueError naming the label.  With
                these, EVERY PERIOD READS ONE PLANE.  "calendar_day": every DAY of the dataset reads the plane labelled with its
                own ``month * 100 + day`` -- the baseline of ``cell_quantiles(period="calendar_day", window=5)``, ETCCDI's TX90p /
                TN10p / WSDI / CSDI as published and xclim's ``percentile_doy`` -- so the threshold changes from day to day inside a
                period (``wagg_row_cell_spells_*``; the kernel reads the listed rows' bytes 1 + K times).  A listed day without
                a plane is ValueError naming the date (29 February in the data against a baseline built with
                ``leap_days="drop"`` while this call keeps leap days); days no period lists need none.  A cell's value is NaN
                if a counted day of the period had a NaN threshold; a cell with no counted day in a period counts 0.  STILL NOT
                BUILT: the percent-of-days form (divide by the period's days), ETCCDI's in-base bootstrap, runs that continue
                across a period boundary.
    stat        "days", "events", "longest" as in :func:`tas_spell_aggregate` (same ``min_length`` rules), or "amount": the sum of
                the variable over the hot days, "excess": the sum of (variable - threshold) over them (``side="below"``:
                threshold - variable); the two sums have no run counter, and a ``min_length`` other than 1 or the default is
                ValueError.  "excess" does not depend on where a Kelvin shift sits.  "AMOUNT" NEEDS THRESHOLDS IN FINAL UNITS
                (``thresholds.shift == 0``: a variable without a shift such as precipitation, or a baseline handed in through
                ``from_array``): the kernel adds ONE offset to a day's value, the field's shift minus the thresholds', so with
                shifted thresholds the sum would be of raw values -- that combination is ValueError, never a wrong number.
    everything else   exactly as in :func:`tas_spell_aggregate`; RUNS ARE TRUNCATED AT PERIOD BOUNDARIES.

    Returns one Dataset with the variable ``varname`` of dims ``("threshold", "period", agglev)``, the coordinate ``threshold`` =
    ``thresholds.levels``, ``attrs["units"]`` = ``"days"`` (days, longest), ``"1"`` (events) or the variable's units (amount,
    excess; ``"C"`` when it carries the Kelvin shift), ``attrs["stat"]``, ``attrs["side"]``, ``attrs["min_length"]``;
    ``results_on_device()`` is honoured; a counted +-inf raises ValueError."""
    from .relative import CellThresholds, resolve_planes
    if not isinstance(thresholds, CellThresholds):
        raise TypeError("thresholds must be a CellThresholds (relative.cell_quantiles or CellThresholds.from_array), got %r"
                        % (type(thresholds).__name__,))
    min_length = _spell_options(stat, side, min_length, ("days", "events", "longest", "amount", "excess"), ("longest", "amount", "excess"))
    if not (planes is None or (isinstance(planes, str) and planes in ("month", "calendar_day")) or callable(planes)):
        raise ValueError("planes must be None, 'month', 'calendar_day' or a callable, got %r" % (planes,))
    if stat == "amount" and thresholds.shift != 0.0:
        raise ValueError("stat='amount' needs thresholds in final units (thresholds.shift == 0, got %r): one offset serves the comparison "
                         "and the sum, so the amount against shifted thresholds would be a sum of raw values; stat='excess' has no such "
                         "limit" % (thresholds.shift,))
    re, var, weights, time_values, labels, _, lists = _period_setup("tas_relative_spell_aggregate", "a relative spell count", ds, tas,
                                                                    weights, period, season, cells, leap_days)
    rmap = pmap = None
    if isinstance(planes, str) and planes == "calendar_day":
        from .periods import period_rows
        from .relative import resolve_row_planes
        rmap = resolve_row_planes(thresholds.labels, time_values, rows=period_rows(time_values, period)[2])
    else:
        pmap = resolve_planes(thresholds.labels, labels, planes)
    grid = (np.asarray(ds.coords["lat"].values), np.asarray(ds.coords["lon"].values))       # (the grid's own labels: `re` carries the table's)
    from . import seasons
    res, rdims, coords, was_xr = seasons._cell_spell_totals(re, tas, aggwt, agglev, weights, backup_aggwt, lists, len(labels), thresholds,
                                                            pmap, min_length, stat, side, season, grid, time_values, cells=cells,
                                                            plane_of_row=rmap)
    rdims, coords = _time_as_period(rdims, coords, labels)
    out = _agg._as_dataset({varname: res}, ("threshold",) + tuple(rdims), dict(coords, threshold=thresholds.levels.copy()), was_xr)
    _spell_attrs(out[varname].attrs, stat, side, min_length, "C" if getattr(var, "_xform", None) is not None else _units(var))
    return out


def _rolling_windows(windows):
    """``windows`` as an int64 vector in the caller's order: at least one integer in 1..16 (duplicates allowed; no bool, no
    float) -- else ValueError"""
    try:
        raw = list(windows)
    except TypeError:
        raise ValueError("windows must be a sequence of integers in 1..16, got %r" % (windows,)) from None
    if len(raw) < 1:
        raise ValueError("windows must be a non-empty sequence of integers in 1..16, got %r" % (windows,))
    for w in raw:
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, np.integer)) or not 1 <= w <= 16:
            raise ValueError("windows must be integers in 1..16 (days), got %r" % (w,))
    return np.array([int(w) for w in raw], dtype=np.int64)


def tas_rolling_aggregate(ds, windows, aggwt, agglev, weights, stat="max", of="mean", tas="tas", varname="tas-rolling",
                          backup_aggwt="areawt", period="year", season=None, cells="all", leap_days="keep"):
    """Rolling-window extremes of a cell's daily values per period (and growing season), aggregated to regions: the greatest or
    least running mean (or sum) over ``W`` consecutive days, for every ``W`` of ``windows`` -- TXx / TNn (``W = 1`` of tasmax /
    tasmin), the hottest or coldest N-day mean of heat-mortality and energy-peak studies, and with ``tas="pr", of="sum",
    windows=[1, 5]`` the ETCCDI Rx1day / Rx5day.  Found on the device in ONE pass per 8 window lengths
    (``wagg_rolling_reduce_*``) instead of a rolling mean, an ``amax`` per period and a full-size temporary per length.

    A window of ``W`` days exists where ``W`` CONSECUTIVE days of one period are all present, in season and not NaN.  WINDOWS
    NEVER REACH ACROSS A PERIOD BOUNDARY: a 5-day window ending on 2 January does not exist in the new year (it is no window of
    the old year either); with ``period="month"`` every month starts anew, and with labels that join the Januaries of several
    years no window reaches from one January into the next.  A missing day, a day out of season and a NaN rule out every window
    that would hold them.  With ``leap_days="drop"`` 28 February and 1 March are consecutive.

    A CELL WITHOUT A VALID WINDOW in a period (a period shorter than ``W``, a season shorter than ``W``, NaN throughout) has NO
    VALUE there: it is NaN for that period and window, and the regional mean treats it as it treats any NaN of a field -- the cell
    adds nothing and its weight stays in the denominator.  This is the one place where "no value" of this family
    reaches the regional result.

    THE REGIONAL VALUE IS THE WEIGHTED MEAN OF THE PER-CELL EXTREMES, not the extreme of the regional mean: every cell takes its
    own hottest ``W`` days, which need not be the same days across a region.

    windows   a non-empty sequence of integers in 1..16 (days) in any order, duplicates allowed; a bool, a float or anything
              outside the range is ValueError.  More than 8 go in several launches.
    stat      "max" or "min", else ValueError.
    of        "mean" (the running mean) or "sum" (the running sum), else ValueError.  For a Kelvin-shifted variable the shift
              is applied once to the result (``W`` times for a sum), never to single days; sums are formed in fp64.
    tas       the variable: a plain field or a Kelvin-shifted one; a power (``tas_poly``) or a degree-day variable is ValueError.
    period    "year", "month" or a label per day; required (None is ValueError).
    season, cells, leap_days   exactly as in :func:`tas_bins_aggregate`.  A counted +-inf raises ValueError.

    Returns one Dataset with the variable ``varname`` of dims ``("window", "period", agglev)`` (the last two in the order the
    period call gives them), the coordinate ``window`` = the lengths as int64 in the caller's order, ``attrs["units"]`` = the
    variable's units (``"C"`` when it carries the Kelvin shift), ``attrs["stat"]`` and ``attrs["of"]``; ``results_on_device()`` is
    honoured."""
    w = _rolling_windows(windows)
    if stat not in ("max", "min"):
        raise ValueError("stat must be 'max' or 'min', got %r" % (stat,))
    if of not in ("mean", "sum"):
        raise ValueError("of must be 'mean' or 'sum', got %r" % (of,))
    re, var, weights, time_values, labels, grid, lists = _period_setup("tas_rolling_aggregate", "a rolling extreme", ds, tas, weights,
                                                                       period, season, cells, leap_days)
    from . import seasons
    res, rdims, coords, was_xr = seasons._rolling_totals(re, tas, aggwt, agglev, weights, backup_aggwt, lists, len(labels), w, stat, of,
                                                         season, grid, time_values, cells=cells)
    rdims, coords = _time_as_period(rdims, coords, labels)
    out = _agg._as_dataset({varname: res}, ("window",) + tuple(rdims), dict(coords, window=w.copy()), was_xr)
    units = "C" if getattr(var, "_xform", None) is not None else _units(var)
    if units is not None:
        out[varname].attrs["units"] = units
    out[varname].attrs["stat"] = stat
    out[varname].attrs["of"] = of
    return out


def _quantile_levels(q):
    """``q`` as a float64 vector in the caller's order: at least one finite number in [0, 1] (duplicates allowed; no bool) --
    else ValueError"""
    try:
        raw = list(q)
    except TypeError:
        raise ValueError("q must be a sequence of numbers in [0, 1], got %r" % (q,)) from None
    if len(raw) < 1:
        raise ValueError("q must be a non-empty sequence of numbers in [0, 1], got %r" % (q,))
    for v in raw:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError("q must be finite numbers in [0, 1], got %r" % (v,))
    return np.array([float(v) for v in raw], dtype=np.float64)


def tas_quantile_aggregate(ds, q, aggwt, agglev, weights, method="linear", tas="tas", varname="tas-quantile", backup_aggwt="areawt",
                           period="year", season=None, cells="all", leap_days="keep"):
    """Per-cell quantiles of the daily values of a period (and growing season), aggregated to regions: the annual (monthly,
    in-season) median, the 5th / 95th / 99th percentile of a cell's days, with ``tas="pr"`` the R95p / R99p thresholds, the
    "typical hot day" of mortality and energy studies -- the order statistics between the extremes of
    :func:`tas_rolling_aggregate` (``windows=[1]``).  Selected exactly on the device in ONE pass per 16 levels
    (``wagg_quantile_select_*``) instead of a ``torch.quantile`` or ``torch.sort`` of a full (T, G) field per period.

    For a cell and a period, the VALID days are those of the period that are present, in season and not NaN; their order does not
    matter.  With ``m`` valid days sorted ``v[0] <= ... <= v[m - 1]``, level ``q`` sits at ``h = (m - 1) * q``: ``lo = floor(h)``,
    ``g = h - lo``, and the value is ``v[lo] + (v[lo + 1] - v[lo]) * g`` (``method="linear"``, NumPy's default), ``v[lo]``
    (``"lower"``) or ``v[lo + 1]`` (``"higher"``; ``v[lo]`` where ``g == 0``), formed in fp64 from the raw elements; a Kelvin shift
    is applied once to the result, never to single days.

    THE REGIONAL VALUE IS THE WEIGHTED MEAN OF THE PER-CELL QUANTILES, not a quantile of the regional mean: every cell takes its
    own 95th-percentile day, which need not be the same day across a region.

    A CELL WITHOUT A VALID DAY in a period (NaN throughout, a season that misses the period) has NO VALUE there: it is NaN for
    that period at every level, and the regional mean treats it as it treats any NaN of a field -- the cell adds nothing and its
    weight stays in the denominator.  A counted +-inf raises ValueError.

    q         a non-empty sequence of finite numbers in [0, 1] in any order, duplicates allowed; a bool, a NaN or anything outside
              is ValueError.  More than 16 go in several launches.
    method    "linear", "lower" or "higher", else ValueError.
    tas       the variable: a plain field or a Kelvin-shifted one; a power (``tas_poly``) or a degree-day variable is ValueError.
    period    "year", "month" or a label per day; required (None is ValueError).  A PERIOD OF MORE THAN 1024 DAYS is ValueError:
              a cell's whole period is held on the chip at once.
    season, cells, leap_days   exactly as in :func:`tas_bins_aggregate`.

    Returns one Dataset with the variable ``varname`` of dims ``("quantile", "period", agglev)`` (the last two in the order the
    period call gives them), the coordinate ``quantile`` = ``q`` as float64 in the caller's order, ``attrs["units"]`` = the
    variable's units (``"C"`` when it carries the Kelvin shift) and ``attrs["method"]``; ``results_on_device()`` is honoured."""
    from ._lib import QUANT_ROWS_MAX
    qv = _quantile_levels(q)
    if method not in ("linear", "lower", "higher"):
        raise ValueError("method must be 'linear', 'lower' or 'higher', got %r" % (method,))
    re, var, weights, time_values, labels, grid, lists = _period_setup("tas_quantile_aggregate", "a period quantile", ds, tas, weights,
                                                                       period, season, cells, leap_days)
    counts = np.diff(lists.row_begin)
    if len(counts) and int(counts.max()) > QUANT_ROWS_MAX:
        worst = int(np.argmax(counts))
        raise ValueError("tas_quantile_aggregate: period %s lists %d days; a period quantile holds at most %d days of a period"
                         % (labels[worst], int(counts[worst]), QUANT_ROWS_MAX))
    max_rows = max(1, int(counts.max()) if len(counts) else 1)
    from . import seasons
    res, rdims, coords, was_xr = seasons._quantile_totals(re, tas, aggwt, agglev, weights, backup_aggwt, lists, len(labels), qv, method,
                                                          max_rows, season, grid, time_values, cells=cells)
    rdims, coords = _time_as_period(rdims, coords, labels)
    out = _agg._as_dataset({varname: res}, ("quantile",) + tuple(rdims), dict(coords, quantile=qv.copy()), was_xr)
    units = "C" if getattr(var, "_xform", None) is not None else _units(var)
    if units is not None:
        out[varname].attrs["units"] = units
    out[varname].attrs["method"] = method
    return out


def validate_edd_snyder_agriculture(ds, thresholds):
    """Drop-in for transformations.py:150-157: ``ds`` has 24,378 ``hierid`` regions and every threshold in ``refTemp`` -- what
    ``snyder_edd_aggregate(..., agglev="hierid")`` returns on the impact-region table.  AssertionError otherwise."""
    assert tuple(ds["hierid"].shape) == (24378,), "hierid dims do not match 24378"
    on_ladder = set(np.asarray(ds["refTemp"].values).ravel().tolist())
    for e in thresholds:
        assert e in on_ladder
