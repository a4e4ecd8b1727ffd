"""Growing-season totals: the reference's per-cell growing-season mask (``climate_toolbox/utils/utils.py:83-153``) as one packed
day-of-year window per grid cell, applied on the device while the field is summed over each period.

Reference (read as text): climate_toolbox/utils/utils.py
  season_boundaries(growing_days)                               :83-110
  get_daily_growing_season_mask(lat, lon, time, growing_days)   :113-153

Its users multiply the daily degree days by the (lat, lon, time) mask, aggregate to regions and sum over the year.  The daily
masked result is linear in the field, and weights and denominators do not depend on time, so

  sum_{t in p} out_masked[t, r] = sum_i w_i * S[p, cell_i] / den_r,
  S[p, c] = sum over the days t of period p on which cell c is in season of f(x[t, c])

with a NaN term counting 0 and its weight staying in the denominator (S6); a day out of season counts 0 in the same way.  ``S``
is the reduce-first period sum of periods.py with one more predicate per cell (``wagg_season_reduce_*``,
csrc/wagg_season.hip); the plan then contracts P rows.  The label work -- the boundaries, the windows, the join of the mask's
grid to the dataset's -- runs here on the host, like _labels.py.

The window of a cell, with ``a = ceil(min_day)`` and ``b = floor(max_day)`` (utils.py:143-149):
  z1 (planting day) is NaN           never in season; the mask value is NaN                        (null window)
  z2 >= z1                           in season on day d iff a <= d <= b
  otherwise (also z2 NaN, z1 given)  in season iff NOT (a <= d <= b): the season wraps the year end and the two boundary days
                                     themselves are out (``1 - mask``); with z2 NaN no day satisfies ``d <= NaN``: all year
packed as include/wagg.h lays it out: bits 0-9 ``a``, 10-19 ``b`` (both clamped to 0..1023), bit 20 invert, bit 21 null; an
interval that is empty is stored as ``a = 1, b = 0``.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import aggregations as _agg, engine as _engine, minixr
from ._labels import _exact_index
from ._layout import _flatten_for_device, _is_device_tensor, _result_dims, _spatial_layout, _to_device
from ._lib import BIN_EDGES_MAX as _BIN_EDGES_MAX, EDD_LADDER_MAX as _EDD_LADDER_MAX, HINGE_MAX as _HINGE_MAX, SEASON_INVERT, SEASON_NULL
from ._lib import SPELL_MAX as _SPELL_MAX
from ._lib import ROLL_MAX_WINDOWS as _ROLL_MAX_WINDOWS
from ._lib import QUANT_MAX as _QUANT_MAX
from ._lib import EXPOSURE_EDGES_MAX as _EXPOSURE_EDGES_MAX
from ._plans import _drop_plan, _plan_for
from ._prepared import PreparedWeights

__all__ = ["season_boundaries", "season_windows", "get_daily_growing_season_mask", "SeasonMask", "SeasonWindows", "day_of_year"]

# ``windows``: int32 (latitude, longitude) packed windows; ``latitude`` / ``longitude``: the growing-days grid's labels, the
# longitudes shifted by -180 and ascending
SeasonWindows = namedtuple("SeasonWindows", ["windows", "latitude", "longitude"])


def _planes(growing_days):
    """(z1, z2, latitude, longitude): planting and harvest day as (latitude, longitude) float64 arrays, the longitudes shifted
    by -180 and sorted (utils.py:86-89; the caller's dataset is left as it is)."""
    if isinstance(growing_days, str):
        from .output import read_netcdf
        growing_days = read_netcdf(growing_days)
    var = growing_days["variable"]
    dims = tuple(var.dims)
    if sorted(dims) != ["latitude", "longitude", "z"]:
        raise ValueError("growing_days needs variable(z, latitude, longitude), got dims %r" % (dims,))
    v = np.transpose(np.asarray(var.values, dtype=np.float64), [dims.index(d) for d in ("z", "latitude", "longitude")])
    if "z" in growing_days.coords:
        z = np.asarray(growing_days.coords["z"].values)
        i1, i2 = np.flatnonzero(z == 1), np.flatnonzero(z == 2)
        if len(i1) != 1 or len(i2) != 1:
            raise KeyError("growing_days needs z = 1 (planting day) and z = 2 (harvest day)")
        z1, z2 = v[i1[0]], v[i2[0]]
    else:
        if v.shape[0] != 2:
            raise ValueError("growing_days needs two z planes: planting day and harvest day")
        z1, z2 = v[0], v[1]
    lat = np.asarray(growing_days.coords["latitude"].values)
    lon = np.asarray(growing_days.coords["longitude"].values) - 180
    order = np.argsort(lon, kind="stable")
    return z1[:, order], z2[:, order], lat, lon[order]


def season_boundaries(growing_days):
    """Drop-in for utils.py:83-110: ``(min_day, max_day)``, the planting / harvest pair of every cell sorted elementwise (NaN
    last, as ``np.sort`` puts it), on the growing-days grid with its longitudes shifted by -180 and sorted.  ``growing_days``:
    a Dataset with ``variable(z, latitude, longitude)`` (z = 1 planting day, z = 2 harvest day) or the path of its file.
    Unlike the reference this does not write the shifted longitudes back into the caller's dataset."""
    z1, z2, lat, lon = _planes(growing_days)
    both = np.sort(np.stack([z1, z2], axis=2), axis=2)
    coords = {"latitude": lat, "longitude": lon}
    return tuple(minixr.DataArray(both[:, :, k], ("latitude", "longitude"), coords=dict(coords, sort=name), name=name)
                 for k, name in enumerate(("min", "max")))


def season_windows(growing_days):
    """One packed int32 window per cell of the growing-days grid (the module docstring has the rule and the packing) as a
    :class:`SeasonWindows` ``(windows, latitude, longitude)``: what ``season=`` of the period calls takes."""
    z1, z2, lat, lon = _planes(growing_days)
    both = np.sort(np.stack([z1, z2], axis=2), axis=2)
    with np.errstate(invalid="ignore"):
        lo, hi = np.ceil(both[:, :, 0]), np.floor(both[:, :, 1])
        null = np.isnan(z1)
        invert = ~(z2 >= z1) & ~null                                   # (a NaN harvest day compares false: the complement)
        empty = ~(lo <= hi) | (hi < 0) | (lo > 1023)                   # (NaN on either side: no day is inside)
    a = np.where(empty, 1, np.clip(np.nan_to_num(lo, nan=1.0), 0, 1023)).astype(np.int32)
    b = np.where(empty, 0, np.clip(np.nan_to_num(hi, nan=0.0), 0, 1023)).astype(np.int32)
    win = a | (b << 10) | np.where(invert, SEASON_INVERT, 0).astype(np.int32) | np.where(null, SEASON_NULL, 0).astype(np.int32)
    return SeasonWindows(win.astype(np.int32), lat, lon)


def day_of_year(time_values):
    """The day of year of every time step: the calendar day (1..366) of datetime64 values, ``v % 1000`` of the YYYYDDD
    integers ``tas_poly`` writes (365-day calendar).  Any other dtype raises ValueError."""
    t = np.asarray(time_values)
    if t.dtype.kind == "M":
        d = t.astype("datetime64[D]")
        return ((d - d.astype("datetime64[Y]").astype("datetime64[D]")).astype(np.int64) + 1).astype(np.int32)
    if t.dtype.kind in "iu":
        return (t.astype(np.int64) % 1000).astype(np.int32)
    raise ValueError("the day of year needs datetime64 or YYYYDDD integer time values, got dtype %s" % t.dtype)


class SeasonMask:
    """What :func:`get_daily_growing_season_mask` returns: the (lat, lon, time) growing-season mask, lazily -- the windows of
    the growing-days grid and the day of year of every time step.  ``.values`` materialises float64 0 / 1 / NaN on the device
    (``wagg_season_mask``); handed to a period call as ``season=`` nothing is materialised at all."""

    dims = ("lat", "lon", "time")

    def __init__(self, windows, time_values):
        self.windows = windows
        self.doy = day_of_year(time_values)
        self.coords = {"lat": minixr.DataArray(windows.latitude, ("lat",)), "lon": minixr.DataArray(windows.longitude, ("lon",)),
                       "time": minixr.DataArray(np.asarray(time_values), ("time",))}

    @property
    def shape(self):
        return tuple(self.windows.windows.shape) + (len(self.doy),)

    @property
    def values(self):
        _engine.require_gpu()
        out = _engine.season_mask(self.doy, self.windows.windows.reshape(-1))
        return out.cpu().numpy().reshape(self.shape)

    def __array__(self, dtype=None, copy=None):
        v = self.values
        return v.astype(dtype) if dtype is not None else v


def get_daily_growing_season_mask(lat, lon, time, growing_days):
    """Drop-in for utils.py:113-153: the mask of the days inside each cell's calendar growing season, dims (lat, lon, time), as
    a lazy :class:`SeasonMask`.  ``growing_days``: the path of the growing-days file (or the Dataset itself).  As in the
    reference ``lat`` and ``lon`` select nothing -- the result lives on the growing-days grid, its longitudes shifted by -180
    and sorted; ``time`` (a coordinate or an array: datetime64, or YYYYDDD integers) gives the day of year."""
    return SeasonMask(season_windows(growing_days), np.asarray(getattr(time, "values", time)))


# ----------------------------------------------------------------------------------------------
# season= of the period calls
# ----------------------------------------------------------------------------------------------
def _as_windows(season):
    if isinstance(season, SeasonMask):
        return season.windows
    if isinstance(season, SeasonWindows):
        return season
    raise TypeError("season must be a SeasonMask (get_daily_growing_season_mask) or the result of season_windows")


def _stored_windows(season, lat, lon, dims, shape, lon_perm):
    """The windows of the dataset's cells in the field's STORED cell order (the order ``_cell_index`` numbers cells in): the
    mask's grid joined to the dataset's ``lat`` / ``lon`` labels by exact equality (KeyError for a cell the mask lacks), then
    laid out like the buffer -- (lat, lon) or (lon, lat), column ``lon_perm[j]`` of the buffer holding longitude label j."""
    sw = _as_windows(season)
    ilat = _exact_index(sw.latitude, np.asarray(lat), "season latitude")
    ilon = _exact_index(sw.longitude, np.asarray(lon), "season longitude")
    if (len(lat), len(lon)) != (shape["lat"], shape["lon"]):
        raise ValueError("the dataset's lat / lon coordinates do not match its field")
    win = np.asarray(sw.windows, dtype=np.int32)[np.ix_(ilat, ilon)]
    stored = np.empty_like(win)
    stored[:, np.arange(len(lon)) if lon_perm is None else np.asarray(lon_perm)] = win
    ia, io, *_ = _spatial_layout(dims)
    return np.ascontiguousarray(stored if ia < io else stored.T).reshape(-1)


def _gridded_field(ds, variable, P, what):
    """``(values, dims)`` of the (time x lat x lon) field that a sum-first call of ``what`` takes; ValueError for anything else"""
    if not (isinstance(ds, _agg.ReindexedDataset) and variable in ds._src_values):
        raise ValueError("%s needs a gridded variable with 'lat' and 'lon' dimensions, got %r" % (what, variable))
    if P == 0:
        raise ValueError("%s needs at least one period" % what)
    values, dims = ds._src_values[variable], ds._src_dims[variable]
    *_, others = _spatial_layout(dims)
    if [dims[i] for i in others] != ["time"]:
        raise ValueError("%s needs a field whose only dimension besides lat / lon is time, got dims %r" % (what, dims))
    return values, dims


def _segment_table(ds, variable, aggwt, agglev, weights, backup_aggwt):
    """``(prepared, w_eff, uniq, codes, cell_idx, G)``: the effective weight and region code of every table row, the sorted
    region labels, and the cell every row reads"""
    prepared = weights if isinstance(weights, PreparedWeights) else None
    if prepared is not None:
        prepared.check(aggwt, agglev, backup_aggwt)
        w_eff, uniq, codes = prepared.w_eff, prepared.uniq.copy(), prepared.codes
    else:
        w_eff = _agg._backup_fill(weights[aggwt].values, weights[backup_aggwt].values)
        uniq, codes = _agg._factorize_labels(np.asarray(weights[agglev].values))
    cell_idx, G = ds._cell_index(variable)
    if len(cell_idx) != len(w_eff):
        raise ValueError("weights has %d rows but the dataset was reindexed with %d" % (len(w_eff), len(cell_idx)))
    return prepared, w_eff, uniq, codes, cell_idx, G


def _stored_season(ds, variable, season, grid, dims, shape, time_values):
    """``(doy, windows)`` of a ``season=`` call, the windows in the field's stored cell order"""
    win = _stored_windows(season, grid[0], grid[1], dims, shape, ds._lon_perms.get(variable))
    doy = day_of_year(time_values)
    if len(doy) != shape["time"]:
        raise ValueError("the dataset's time coordinate has %d steps, the field %d" % (len(doy), shape["time"]))
    return doy, win


def _time_by_cell(buf, dims):
    """the field as a (time, gridcell) device tensor: uploaded whole if it is host-resident, transposed on the device if it is
    stored (gridcell, time)"""
    X2, layout, _, _ = _flatten_for_device(buf, dims)
    Xd = _to_device(X2)
    return Xd if layout == "TG" else _engine.relayout(Xd, [1, 0])


def _check_cells(cells):
    if cells not in ("all", "referenced"):
        raise ValueError("cells must be 'all' or 'referenced', got %r" % (cells,))
    return cells


def _compact_cells_of(plan, dtype):
    """``cells="referenced"``: the cells of the plan's compact row (``SparsePlan.compact_cells``), or None where the call falls
    back to whole rows -- a dense-family plan, a plan without the quads map, a packed row above 80 % of the row"""
    if not isinstance(plan, _engine.SparsePlan):
        return None
    pos = plan.compact_cells(dtype)
    return None if pos is None or 5 * len(pos) > 4 * plan.G else pos


def _referenced_rows(values, second, dims, make_plan):
    """``cells="referenced"`` of the sum-first routes: ``(plan, X, H, cell_of_pos)`` -- the leased plan (``make_plan(dtype)``)
    and the field(s) as (time, Gq) device matrices holding only the quads the table references (``engine.pack_rows``: a
    host-resident field is packed by host threads and only the quads cross PCIe, a (gridcell, time) one is transposed on the
    device first), column j being cell ``cell_of_pos[j]``.  ``cell_of_pos`` None: the call falls back (:func:`_compact_cells_of`)
    and X / H are the whole (time, gridcell) rows of ``_time_by_cell``.  ``second``: tasmax, or None."""
    X2, layout, _, _ = _flatten_for_device(values, dims)
    H2 = None if second is None else _flatten_for_device(second, dims)[0]
    if H2 is not None and (tuple(H2.shape) != tuple(X2.shape) or H2.dtype != X2.dtype):
        raise ValueError("tasmin and tasmax must have the same shape and dtype")
    plan = make_plan(X2.dtype)
    try:
        pos = _compact_cells_of(plan, X2.dtype)
        if pos is None or layout != "TG":
            whole = lambda a: None if a is None else (_to_device(a) if layout == "TG" else _engine.relayout(_to_device(a), [1, 0]))
            X2, H2 = whole(X2), whole(H2)
            if pos is None:
                return plan, X2, H2, None
        packed = _engine.pack_rows(plan, X2, H2)
        return plan, packed[:, :len(pos)], (None if H2 is None else packed[:, len(pos):]), pos
    except BaseException:
        plan._lease.release()
        raise


def _result_coords(ds, rdims, agglev, uniq):
    carried = ds.coords
    coords = {d: np.asarray(carried[d].values) for d in rdims if d != agglev and d in carried and tuple(carried[d].dims) == (d,)}
    coords[agglev] = uniq
    return coords


def _leased_rows(ds, variable, aggwt, agglev, weights, backup_aggwt, values, dims, second, season, grid, time_values, cells):
    """The set-up every sum-first route here shares behind its own checks of the variable: the segment table, the season's
    ``(doy, windows)`` in stored cell order (``season`` None: None, None), and the plan, LEASED, beside the field on the device --
    whole (time, gridcell) rows, or for ``cells="referenced"`` the packed rows of :func:`_referenced_rows` (``second``: tasmax
    or None, packed along) with the windows of those cells.  Returns ``(plan, Xd, Hd, pos, doy, win, uniq)``; ``Hd`` None: a
    second field is still to come over whole.  The caller releases ``plan._lease``."""
    prepared, w_eff, uniq, codes, cell_idx, G = _segment_table(ds, variable, aggwt, agglev, weights, backup_aggwt)
    shape = dict(zip(dims, tuple(values.shape)))
    ia, io, *_ = _spatial_layout(dims)
    doy, win = (None, None) if season is None else _stored_season(ds, variable, season, grid, dims, shape, time_values)
    _engine.require_gpu()
    make_plan = lambda dtype: _plan_for(cell_idx, codes, w_eff, G, len(uniq), shape["lon"] if ia < io else shape["lat"],
                                        is_f32=str(dtype).endswith("float32"), layout="TG", prepared=prepared)
    Hd = pos = None
    if cells == "referenced":
        plan, Xd, Hd, pos = _referenced_rows(values, second, dims, make_plan)
        if pos is not None and win is not None:
            win = win[pos]
    else:
        Xd = _time_by_cell(values, dims)
        plan = make_plan(Xd.dtype)
    return plan, Xd, Hd, pos, doy, win, uniq


def _second_field(Xd, Hd, second, dims):
    """tasmax beside ``Xd``: the packed ``Hd``, else ``second`` brought over whole; ValueError unless it matches ``Xd``"""
    Hd = _time_by_cell(second, dims) if Hd is None else Hd
    if Hd.shape != Xd.shape or Hd.dtype != Xd.dtype:
        raise ValueError("tasmin and tasmax must have the same shape and dtype")
    return Hd


def _season_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, powers, offset, season, grid, time_values,
                   cells="all"):
    """The one route of a ``season=`` call: sum first (``wagg_season_reduce_*``), then contract P rows on whatever plan serves
    the table.  Returns what ``periods._reduce_first`` returns; raises where that one would fall back -- there is no daily masked
    route to fall back to.  ``cells="referenced"``: all of it on the packed rows of :func:`_referenced_rows`."""
    from . import periods as _periods
    values, dims = _gridded_field(ds, variable, P, "season=")
    xform, edd = ds._xforms.get(variable), ds._edds.get(variable)
    if (powers is not None or edd is not None) and xform is not None:
        raise ValueError("variable %r already carries a lazy transform" % (variable,))
    single = powers is None
    if powers is None and xform is not None:
        offset, powers = xform[0], [xform[1]]
    if powers is not None and (max(powers) - min(powers) >= 4 or max(powers) > 16):
        raise ValueError("season= takes powers within 1..16 that span at most four consecutive ones, got %r" % (powers,))
    if edd is not None and len(edd[2]) > 4:
        raise ValueError("season= takes degree-day combinations of at most four thresholds")
    plan, Xd, Hd, pos, doy, win, uniq = _leased_rows(ds, variable, aggwt, agglev, weights, backup_aggwt, values, dims,
                                                     None if edd is None else edd[0], season, grid, time_values, cells)
    try:
        rb, rw = lists(Xd.device)
        if edd is not None:
            Hd = _second_field(Xd, Hd, edd[0], dims)
            field, status = _engine.season_reduce(Xd, rb, rw, doy, win, X2=Hd, edd=(edd[1], [e for _, e in edd[2]]), checked=True)
        elif powers is not None:
            lo, hi = int(min(powers)), int(max(powers))
            field, status = _engine.season_reduce(Xd, rb, rw, doy, win, poly=(offset, lo, hi - lo + 1), checked=True)
        else:
            field, status = _engine.season_reduce(Xd, rb, rw, doy, win, checked=True)
        if int(status.item()) & 1:
            raise ValueError("season=: an in-season value of %r is +-inf (in the data, or a power that overflows); season totals "
                             "have no daily route that could give it the daily treatment" % (variable,))
        rdims = _result_dims(dims, agglev)
        res = _periods._contract(plan, field, P, len(uniq), edd, powers, rdims, agglev,
                                 _agg._device_results_wanted() and _is_device_tensor(values) and not ds._was_xarray, compact=pos is not None)
        if res is None:
            raise ValueError("season=: the season totals of %r overflow the element type (the dense-family plan met +-inf)" % (variable,))
    except _engine.WaggError:
        _drop_plan(plan)
        raise
    finally:
        plan._lease.release()
    return (res[0] if single or edd is not None else res), rdims, _result_coords(ds, rdims, agglev, uniq), ds._was_xarray


def _degree_day_variable(ds, variable, what):
    """``(tasmax, offset)`` of a degree-day variable (its own terms are ignored); ValueError for any other"""
    edd = ds._edds.get(variable)
    if edd is None or ds._xforms.get(variable) is not None:
        raise ValueError("%s needs a degree-day variable, got %r" % (what, variable))
    return edd[0], edd[1]


def _plain_variable(ds, variable, what):
    """``(None, offset)`` of a plain temperature variable or one shifted by ``convert_kelvin_to_celsius`` (the offset is the
    shift); ValueError for a power or a degree-day variable"""
    xform = ds._xforms.get(variable)
    if ds._edds.get(variable) is not None or (xform is not None and xform[1] != 1):
        raise ValueError("%s needs a plain (or Kelvin-shifted) temperature variable, got %r" % (what, variable))
    return None, 0.0 if xform is None else float(xform[0])


def _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells, name, of, rule,
                    launches, pass_cells=False):
    """The sum-first route of the grouped statistics (ladder, bins, hinges, exposure bins, spells, rolling extremes, period quantiles): every launch reduces its planes per period
    first, then one apply per launch contracts its planes * P rows on whatever plan serves the table.  ``name`` / ``of``: the statistic in
    the messages ("bin count" / "bins"); ``rule(ds, variable, what)``: ``(second field or None, offset)`` of a variable the
    statistic takes, ValueError for any other; ``launches``: an iterable, consumed as the launches run, of
    ``reduce(Xd, Hd, rb, rw, offset, **season)`` -> ``(planes, status)``, each one engine call on its cut of the parameter
    list.  ``season`` None: every day counts.  ``cells="referenced"``: all of it on the packed rows of :func:`_referenced_rows`.
    ``pass_cells``: a launch also gets ``cells=`` -- None for whole rows, else the grid cell of every packed column (a
    statistic with a per-cell parameter takes its columns by it).
    Returns ``(stack, rdims, coords, was_xarray)`` like :func:`_season_totals`, ``stack`` being the (planes, P | R, R | P)
    results of all launches in order."""
    from . import periods as _periods
    values, dims = _gridded_field(ds, variable, P, "a " + name)
    second, offset = rule(ds, variable, "a " + name)
    plan, Xd, Hd, pos, doy, win, uniq = _leased_rows(ds, variable, aggwt, agglev, weights, backup_aggwt, values, dims, second, season,
                                                     grid, time_values, cells)
    try:
        rb, rw = lists(Xd.device)
        if second is not None:
            Hd = _second_field(Xd, Hd, second, dims)
        rdims = _result_dims(dims, agglev)
        keep_dev = _agg._device_results_wanted() and _is_device_tensor(values) and not ds._was_xarray
        res = []
        for reduce in launches:
            field, status = reduce(Xd, Hd, rb, rw, offset, doy=doy, windows=win, checked=True, **({"cells": pos} if pass_cells else {}))
            if int(status.item()) & 1:
                raise ValueError("%s: a counted value of %r is +-inf; period totals of %s have no daily route that could give it the "
                                 "daily treatment" % (name, variable, of))
            got = _periods._contract(plan, field, P, len(uniq), None, None, rdims, agglev, keep_dev, planes=True, compact=pos is not None)
            if got is None:
                raise ValueError("%s: the totals of %r overflow the element type (the dense-family plan met +-inf)" % (name, variable))
            res.extend(got)
    except _engine.WaggError:
        _drop_plan(plan)
        raise
    finally:
        plan._lease.release()
    stack = _engine.require_gpu().stack(res) if keep_dev else np.stack(res)
    return stack, rdims, _result_coords(ds, rdims, agglev, uniq), ds._was_xarray


def _ladder_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, ladder, season, grid, time_values, cells="all"):
    """Period totals of the degree days of ``variable`` (a degree-day variable; its own terms are ignored) at EVERY threshold of
    ``ladder`` (``wagg_edd_ladder_reduce_*``, up to 64 thresholds a launch) through :func:`_grouped_totals`; ``stack`` is the
    (n_thr, P | R, R | P) results in the ladder's order."""
    def launches():
        for k0 in range(0, len(ladder), _EDD_LADDER_MAX):
            thr = [float(e) for e in ladder[k0:k0 + _EDD_LADDER_MAX]]
            yield lambda X, H, rb, rw, offset, **kw: _engine.edd_ladder_reduce(X, H, rb, rw, offset, thr, **kw)

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells,
                           "degree-day ladder", "a ladder", _degree_day_variable, launches())


def _bin_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, edges, season, grid, time_values, cells="all"):
    """Period totals of the days ``variable`` spends in every bin ``[edges[k], edges[k + 1])`` (``wagg_bin_days_reduce_*``, up to
    64 bins a launch) through :func:`_grouped_totals`.  ``variable``: a plain temperature variable, or one shifted by
    ``convert_kelvin_to_celsius`` (the edges are then in degrees C); a power or a degree-day variable is ValueError.  ``stack``
    is the (n_bins, P | R, R | P) results in bin order."""
    def launches():
        for k0 in range(0, len(edges) - 1, _BIN_EDGES_MAX - 1):                  # (consecutive launches share an edge)
            part = [float(e) for e in edges[k0:k0 + _BIN_EDGES_MAX]]
            yield lambda X, H, rb, rw, offset, **kw: _engine.bin_days_reduce(X, rb, rw, offset, part, **kw)

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells, "bin count",
                           "bins", _plain_variable, launches())


def _exposure_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, edges, season, grid, time_values, cells="all"):
    """Period totals of the time the daily sinusoid of ``variable`` (a degree-day variable: tasmin with its tasmax; its own terms
    are ignored) spends in every bin ``[edges[k], edges[k + 1])`` (``wagg_exposure_reduce_*``, up to 64 bins a launch) through
    :func:`_grouped_totals`; ``stack`` is the (n_bins, P | R, R | P) results in bin order."""
    def launches():
        for k0 in range(0, len(edges) - 1, _EXPOSURE_EDGES_MAX - 1):             # (consecutive launches share an edge)
            part = [float(e) for e in edges[k0:k0 + _EXPOSURE_EDGES_MAX]]
            yield lambda X, H, rb, rw, offset, **kw: _engine.exposure_reduce(X, H, rb, rw, offset, part, **kw)

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells,
                           "exposure total", "exposure bins", _degree_day_variable, launches())


def _hinge_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, knots, power, side, tail, season, grid, time_values,
                  cells="all"):
    """Period totals of the hinges ``max(+-(variable - knots[j]), 0) ** power`` at EVERY knot (``wagg_hinge_reduce_*``, up to 64
    knots a launch) through :func:`_grouped_totals`.  ``variable``: as for :func:`_bin_totals` (the knots are in degrees C for a
    shifted one, and the shift is the kernel's offset).  ``tail``: None, or ``(two tail knots, a, b)`` with a coefficient per
    knot (``engine.hinge_reduce``).  ``stack`` is the (n_knots, P | R, R | P) results in the knots' order."""
    def launches():
        for k0 in range(0, len(knots), _HINGE_MAX):
            sl = slice(k0, k0 + _HINGE_MAX)
            part, cut = [float(k) for k in knots[sl]], None if tail is None else (tail[0], tail[1][sl], tail[2][sl])
            yield lambda X, H, rb, rw, offset, **kw: _engine.hinge_reduce(X, rb, rw, offset, part, power=power, side=side, tail=cut, **kw)

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells, "hinge total",
                           "hinges", _plain_variable, launches())


def _spell_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, thresholds, min_length, stat, side, season, grid,
                  time_values, cells="all", span="period"):
    """Period totals of the spell statistic ``stat`` of ``variable`` at EVERY threshold (``wagg_spell_reduce_*``, up to 64
    thresholds a launch) through :func:`_grouped_totals`.  ``variable``: as for :func:`_bin_totals` (the thresholds are in degrees
    C for a shifted one).  A run ends with its period's list: the regional value is the weighted mean of per-cell counts of runs
    truncated there -- with ``span="record"`` (``wagg_spell_span_*``) of runs that continue across the boundaries, as
    ``engine.spell_reduce`` defines them.  ``stack`` is the (n_thr, P | R, R | P) results in the thresholds' order."""
    def launches():
        for k0 in range(0, len(thresholds), _SPELL_MAX):
            part = [float(t) for t in thresholds[k0:k0 + _SPELL_MAX]]
            yield lambda X, H, rb, rw, offset, **kw: _engine.spell_reduce(X, rb, rw, offset, part, min_length=min_length, stat=stat,
                                                                          side=side, span=span, **kw)

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells, "spell count",
                           "spells", _plain_variable, launches())


def _cell_spell_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, thresholds, plane_of_period, min_length, stat, side,
                       season, grid, time_values, cells="all", plane_of_row=None):
    """Period totals of the spell / exceedance statistic ``stat`` of ``variable`` against the PER-CELL thresholds of a
    ``relative.CellThresholds`` (``wagg_cell_spells_*``, up to 64 levels a launch) through :func:`_grouped_totals`.  ``variable``:
    as for :func:`_bin_totals`; ``grid``: the dataset's own ``(lat, lon)`` labels (also without a season), to which the
    thresholds' grid is joined by exact labels in the field's stored cell order, converted to the field's dtype once; with
    ``cells="referenced"`` the packed columns are taken on the device.  ``plane_of_period``: the plane index of every period; or
    None with ``plane_of_row``: the plane index of every day (``wagg_row_cell_spells_*``: calendar-day thresholds).
    The kernel's offset is the field's shift minus the thresholds' own -- exactly 0 when both come from one Kelvin variable.  A
    cell whose threshold is NaN is NaN there, which the contraction treats as any NaN of a field.  ``stack`` is the (K, P | R,
    R | P) results in the levels' order."""
    from ._lib import CELL_SPELL_MAX
    from .relative import cell_spell_reduce
    state = {}

    def stored(X, cells_of_pos):
        if "thr" not in state:                       # (behind _gridded_field's checks: once, whatever the number of launches)
            thr = thresholds.stored(grid[0], grid[1], ds._src_dims[variable], ds._lon_perms.get(variable), X.dtype, X.device)
            state["thr"] = thr if cells_of_pos is None else _engine.take_axis(thr, 2, cells_of_pos)
            pmap = plane_of_period if plane_of_row is None else plane_of_row
            state["map"] = _engine.require_gpu().from_numpy(np.ascontiguousarray(pmap, dtype=np.int32)).to(X.device)
        return state["thr"], state["map"]

    def launches():
        for k0 in range(0, thresholds.K, CELL_SPELL_MAX):
            def reduce(X, H, rb, rw, offset, cells=None, k0=k0, **kw):
                thr, pmap = stored(X, cells)
                which = {"plane_of_period": pmap} if plane_of_row is None else {"plane_of_row": pmap}
                return cell_spell_reduce(X, rb, rw, offset - thresholds.shift, thr[k0:k0 + CELL_SPELL_MAX], min_length=min_length,
                                         stat=stat, side=side, **which, **kw)
            yield reduce

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, None if season is None else grid,
                           time_values, cells, "relative spell count", "relative spells", _plain_variable, launches(), pass_cells=True)


def _rolling_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, lengths, stat, of, season, grid, time_values,
                    cells="all"):
    """Period extremes of the running ``of`` ("mean" / "sum") of ``variable`` over EVERY window length of ``lengths``
    (``wagg_rolling_reduce_*``, up to 8 lengths a launch) through :func:`_grouped_totals`.  ``variable``: as for
    :func:`_bin_totals`.  A window ends with its period's list; a cell without a valid window in a period is NaN there, which the
    contraction treats as any NaN of a field (it counts 0, its weight stays in the denominator: DESIGN.md, S6).  ``stack`` is the
    (n_win, P | R, R | P) results in the lengths' order."""
    def launches():
        for k0 in range(0, len(lengths), _ROLL_MAX_WINDOWS):
            part = [int(w) for w in lengths[k0:k0 + _ROLL_MAX_WINDOWS]]
            yield lambda X, H, rb, rw, offset, **kw: _engine.rolling_reduce(X, rb, rw, offset, part, stat=stat, of=of, **kw)

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells,
                           "rolling extreme", "rolling windows", _plain_variable, launches())


def _quantile_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, q, method, max_rows, season, grid, time_values,
                     cells="all"):
    """Per-cell quantiles of ``variable`` over the days of every period at EVERY level of ``q`` (``wagg_quantile_select_*``, up
    to 16 levels a launch) through :func:`_grouped_totals`.  ``variable``: as for :func:`_bin_totals`; ``max_rows``: the longest
    period list, which the caller knows from the host lists.  A cell without a valid day in a period is NaN there, which the
    contraction treats as any NaN of a field (it counts 0, its weight stays in the denominator: DESIGN.md, S6).  ``stack`` is the
    (n_q, P | R, R | P) results in the levels' order."""
    def launches():
        for k0 in range(0, len(q), _QUANT_MAX):
            part = [float(v) for v in q[k0:k0 + _QUANT_MAX]]
            yield lambda X, H, rb, rw, offset, **kw: _engine.quantile_select(X, rb, rw, offset, part, method=method, max_rows=max_rows, **kw)

    return _grouped_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, season, grid, time_values, cells,
                           "period quantile", "quantiles", _plain_variable, launches())
