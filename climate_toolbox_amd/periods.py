"""Period totals of the regional aggregates: sums over calendar years, year-months or caller-given labels, on the device.

The reference defines its degree-day measures as period totals (``EDD_P = sum of EDD_d over the days d of P``,
transformations.py:17-19) and ``tas_poly`` relabels time to ``YYYYDDD`` so that a 365-day year can be summed next; its
users take the daily ``(T x R)`` result and sum it themselves.  Here the sum runs on the GPU (``wagg_period_reduce_*``,
csrc/wagg_period.hip), on either side of the aggregation -- it is linear in the field, and weights and denominators do not
depend on time:

  reduce-first      the rows of X (with the lazy transform evaluated per cell and day) are summed per period first, the plan
                    then contracts P rows instead of T.  +-inf in the transformed data (the kernel's status word) sends the
                    call down the other route, which keeps the daily path's treatment of it.
  aggregate-first   the daily path as it is, then the (T x R) result is summed per period with NaN propagating; (P x R)
                    leaves the device instead of (T x R).

DEFINED SEMANTICS: the result equals the sum, over each period's rows, of the daily result.  A NaN daily value (a region
whose denominator is zero) makes the period NaN: it is a plain sum, which does not skip NaN.
"""
from __future__ import annotations

import numpy as np

from . import aggregations as _agg, engine as _engine
from ._layout import _flatten_for_device, _is_device_tensor, _result_dims, _spatial_layout, _to_device
from ._pinned import _to_host
from ._plans import _drop_plan, _plan_for
from ._prepared import PreparedWeights
from .engine import DensePlan, SparsePlan

__all__ = ["weighted_aggregate_grid_to_regions_periods", "period_rows"]

_MONTH_ENDS_365 = np.cumsum([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])     # last day number of each month, no leap day

# Plan families whose AUTOMATIC route is reduce-first, for device-resident (time, gridcell) fields; everything else takes
# aggregate-first.  The rule that decides it: a family stays here only if tools/period_timing.py finds
# its reduce-first median ahead of aggregate-first by more than the larger min-max spread of the two.  Not measured yet:
# "dense" stands by reasoning alone (T rows of matrix work become P; a segment-table plan reads only referenced lines).
REDUCE_FIRST_FAMILIES = frozenset({"dense"})


def _year_month(time_values):
    """(year, month) per time step, from datetime64 values or from the YYYYDDD integers of tas_poly (365-day calendar)."""
    t = np.asarray(time_values)
    if t.dtype.kind == "M":
        months = t.astype("datetime64[M]").astype(np.int64)
        return months // 12 + 1970, months % 12 + 1
    if t.dtype.kind in "iu":
        t = t.astype(np.int64)
        year, day = t // 1000, t % 1000
        if len(t) and (year.min() < 1 or day.min() < 1 or day.max() > 365):
            raise ValueError("integer time values must be YYYYDDD with DDD in 1..365 (what tas_poly writes)")
        return year, np.searchsorted(_MONTH_ENDS_365, day, side="left") + 1
    raise ValueError("'year' / 'month' need datetime64 or YYYYDDD integer time values, got dtype %s" % t.dtype)


def period_rows(time_values, period):
    """Which rows make up which period: ``(labels, row_begin, rows)`` -- the P labels in ascending order and the rows of
    period p, in time order, as ``rows[row_begin[p]:row_begin[p + 1]]`` (CSR).

    period   "year": one period per calendar year, labelled by the year; "month": one per year-month, labelled
             ``year * 100 + month``; or a length-T array of labels: rows with equal labels form a period, a negative integer
             or ``None`` drops the row.  Anything else raises ValueError.
    time_values  datetime64, or the YYYYDDD integers ``tas_poly`` produces (year = v // 1000, month from the day number on
             the 365-day calendar).  On datetime64 time every day counts, 29 February included: it is only ever missing
             because ``tas_poly`` removed it before."""
    T = len(np.asarray(time_values))
    if isinstance(period, str):
        if period not in ("year", "month"):
            raise ValueError("period must be 'year', 'month' or an array of %d labels, got %r" % (T, period))
        year, month = _year_month(time_values)
        lab = year if period == "year" else year * 100 + month
        keep = np.ones(T, dtype=bool)
    else:
        if period is None or np.ndim(period) != 1 or len(period) != T:
            raise ValueError("period must be 'year', 'month' or an array of %d labels" % T)
        lab = np.asarray(period)
        if lab.dtype == object:
            keep = np.array([v is not None for v in lab], dtype=bool)
            ints = [isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in lab[keep]]
            if len(ints) and all(ints):
                lab = np.where(keep, lab, -1).astype(np.int64)
        elif lab.dtype.kind == "f":
            keep = ~np.isnan(lab)
        else:
            keep = np.ones(T, dtype=bool)
        if lab.dtype.kind in "iuf":
            keep = keep & (np.where(keep, lab, 0) >= 0)
        elif lab.dtype.kind not in "OUSM":
            raise ValueError("period labels must be integers, strings or datetimes, got dtype %s" % lab.dtype)
    kept = np.flatnonzero(keep)
    vals = lab[kept]
    if vals.dtype == object:
        try:
            vals = np.array(vals.tolist())
        except Exception:
            raise ValueError("period labels of mixed types cannot be ordered") from None
        if vals.dtype == object or vals.ndim != 1:
            raise ValueError("period labels of mixed types cannot be ordered")
    labels, inv = np.unique(vals, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    row_begin = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(labels)))]).astype(np.int64)
    return labels, row_begin, kept[order].astype(np.int64)


def _sum_time_axis(arr, axis, lists, P, keep_dev):
    """``arr`` (NumPy array or CUDA tensor) with its ``axis`` (time, T rows) replaced by the P period totals; NaN propagates."""
    on_dev = _is_device_tensor(arr)
    if on_dev:
        t = arr.movedim(axis, 0)
        t = t if t.is_contiguous() else _engine.relayout(t)
    else:
        t = _engine.upload(np.ascontiguousarray(np.moveaxis(np.asarray(arr), axis, 0)))
    rest = tuple(t.shape[1:])
    rb, rw = lists(t.device)
    out, _ = _engine.period_reduce(t.reshape(t.shape[0], int(np.prod(rest, dtype=np.int64))), rb, rw, keep_nan=True, checked=True)
    out = out[0].reshape((P,) + rest)
    if on_dev and keep_dev:
        return out.movedim(0, axis)
    return np.moveaxis(_to_host(out), 0, axis)


def _contract(plan, field, P, R, edd, powers, rdims, agglev, keep_dev, planes=False, compact=False):
    """The (planes, P, G) period sums of a field through the leased ``plan``: the list of (P, R) results (in ``rdims`` order;
    device tensors when ``keep_dev``), or None when a dense-family plan met +-inf.  ``planes``: every plane is a result of its
    own, in order (a degree-day ladder) -- nothing is combined or picked.  ``compact``: the sums are (planes, P, Gq) sums of
    packed rows (``cells="referenced"``; a segment-table plan), contracted through the plan's quads-only cell table."""
    K = field.shape[0]
    flat = field.reshape(K * P, field.shape[2])
    if compact:
        out = plan.apply(flat, layout="TG", out_layout="TR", compact=True)
    else:
        out = plan.apply(flat) if isinstance(plan, DensePlan) else plan.apply(flat, layout="TG", out_layout="TR")
    if isinstance(plan, DensePlan) and plan.saw_inf():
        return None
    stack = out.reshape(K, P, R)
    if planes:
        outs = list(stack)
    elif edd is not None:
        coefs = [c for c, _ in edd[2]]
        outs = [stack[0] if coefs == [1.0] else _engine.combine_planes(stack, coefs)]
    elif powers is not None:
        lo = int(min(powers))
        outs = [stack[int(p) - lo] for p in powers]
    else:
        outs = [stack[0]]
    if rdims.index("time") > rdims.index(agglev):
        outs = [o.transpose(0, 1) for o in outs]
    res = [o if keep_dev else _to_host(o.contiguous()) for o in outs]
    if isinstance(plan, SparsePlan):
        if not keep_dev:
            plan.status()
        else:
            pending = getattr(_agg._TLS, "unchecked_plans", None)
            if pending is not None and not any(p is plan for p in pending):
                pending.append(plan)
    return res


def _reduce_first(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, powers, offset, force, cells="all"):
    """The reduce-first route; None when this call cannot (or, unless forced, should not) take it, or met +-inf.
    ``cells="referenced"``: the field(s) are packed to the quads the table references first (``engine.pack_rows``), summed with
    n = Gq and contracted through the plan's quads-only cell table -- where the plan has one (seasons._compact_cells_of)."""
    if not (isinstance(ds, _agg.ReindexedDataset) and variable in ds._src_values):
        return None
    values, dims = ds._src_values[variable], ds._src_dims[variable]
    *_, others = _spatial_layout(dims)
    if P == 0 or [dims[i] for i in others] != ["time"] or not (force or cells == "referenced" or _is_device_tensor(values)):
        return None
    xform, edd = ds._xforms.get(variable), ds._edds.get(variable)
    if (powers is not None or edd is not None) and xform is not None:
        raise ValueError("variable %r already carries a lazy transform" % (variable,))
    single = powers is None
    if powers is None and xform is not None:
        offset, powers = xform[0], [xform[1]]
    if powers is not None and (max(powers) - min(powers) >= 4 or max(powers) > 16):
        return None
    if edd is not None and len(edd[2]) > 4:
        return None
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
    X2, layout, _, _ = _flatten_for_device(values, dims)
    if layout != "TG":
        return None
    shape = dict(zip(dims, tuple(values.shape)))
    ia, io, *_ = _spatial_layout(dims)
    _engine.require_gpu()
    plan = _plan_for(cell_idx, codes, w_eff, G, len(uniq), shape["lon"] if ia < io else shape["lat"],
                     is_f32=str(X2.dtype).endswith("float32"), layout=layout, prepared=prepared)
    try:
        family = "dense" if isinstance(plan, DensePlan) else "segment"
        pos = None
        if cells == "referenced":
            from .seasons import _compact_cells_of
            pos = _compact_cells_of(plan, X2.dtype)
        if pos is None and not force and (family not in REDUCE_FIRST_FAMILIES or not _is_device_tensor(values)):
            return None                              # (also cells="referenced" on a plan that cannot pack: as with "all")
        H2 = None if edd is None else _flatten_for_device(edd[0], dims)[0]
        if H2 is not None and (H2.shape != X2.shape or H2.dtype != X2.dtype):
            raise ValueError("tasmin and tasmax must have the same shape and dtype")
        if pos is not None:
            packed = _engine.pack_rows(plan, X2, H2)
            Xd, Hd = packed[:, :len(pos)], (None if H2 is None else packed[:, len(pos):])
        else:
            Xd, Hd = _to_device(X2), (None if H2 is None else _to_device(H2))
        rb, rw = lists(Xd.device)
        if edd is not None:
            field, status = _engine.period_reduce(Xd, rb, rw, X2=Hd, edd=(edd[1], [e for _, e in edd[2]]), checked=True)
        elif powers is not None:
            lo, hi = int(min(powers)), int(max(powers))
            field, status = _engine.period_reduce(Xd, rb, rw, poly=(offset, lo, hi - lo + 1), checked=True)
        else:
            field, status = _engine.period_reduce(Xd, rb, rw, checked=True)
        if int(status.item()) & 1:
            return None                              # +-inf somewhere: the daily path decides what it means (S6)
        res = _contract(plan, field, P, len(uniq), edd, powers, _result_dims(dims, agglev), agglev,
                        _agg._device_results_wanted() and _is_device_tensor(values) and not ds._was_xarray, compact=pos is not None)
        if res is None:
            return None                              # (finite days whose total overflows fp32)
        rdims = _result_dims(dims, agglev)
    except _engine.WaggError:
        _drop_plan(plan)
        raise
    finally:
        plan._lease.release()
    carried = ds.coords
    coords = {d: np.asarray(carried[d].values) for d in rdims if d != agglev and d in carried and tuple(carried[d].dims) == (d,)}
    coords[agglev] = uniq
    return (res[0] if single or edd is not None else res), rdims, coords, ds._was_xarray


def _aggregate_periods(ds, variables, aggwt, agglev, weights, backup_aggwt, period, time_values, powers=None, offset=0.0, route=None,
                       season=None, grid=None, cells="all"):
    """Body of the period calls.  ``ds``: a reindexed dataset; ``variables``: the name to aggregate (``powers`` None) or the
    result names, one per power of variable "tas".  ``season`` (with ``grid`` = the dataset's own lat / lon labels): only
    in-season days count (seasons.py).  ``cells``: "all", or "referenced" -- sum first, on the quads the table references
    only.  Returns the Dataset with ``time`` replaced by ``period``."""
    if route not in (None, "reduce_first", "aggregate_first"):
        raise ValueError("_route must be None, 'reduce_first' or 'aggregate_first'")
    _check_cells(cells, route)
    if season is not None and route is not None:
        raise ValueError("_route cannot be combined with season=: season totals always sum the field first")
    labels, row_begin, rows = period_rows(time_values, period)
    P = len(labels)
    variable = variables if powers is None else "tas"
    cache = {}

    def lists(device):
        key = str(device)
        if key not in cache:
            cache[key] = _engine.period_lists(row_begin, rows, len(np.asarray(time_values)), device=device)
        return cache[key]

    got = None
    if season is not None:
        from . import seasons
        got = seasons._season_totals(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, powers, offset, season, grid,
                                     time_values, cells=cells)
    elif route != "aggregate_first":
        got = _reduce_first(ds, variable, aggwt, agglev, weights, backup_aggwt, lists, P, powers, offset, route == "reduce_first",
                            cells=cells)
        if got is None and route == "reduce_first" and not _reduce_first_possible(ds, variable, powers):
            raise ValueError("reduce-first needs a (time, gridcell) field whose only other dimension is time")
    if got is None:
        keep_dev = _agg._device_results_wanted()
        with _agg.results_on_device():
            res, rdims, coords, was_xr = _agg._aggregate_core(ds, variable, aggwt, agglev, weights, backup_aggwt, powers=powers,
                                                              offset=offset)
        if "time" not in rdims:
            raise ValueError("variable %r has no 'time' dimension to sum over" % (variable,))
        ax = rdims.index("time")
        many = isinstance(res, list)
        res = [_sum_time_axis(r, ax, lists, P, keep_dev and not was_xr) for r in (res if many else [res])]
        got = (res if many else res[0]), rdims, coords, was_xr
    res, rdims, coords, was_xr = got
    rdims = tuple("period" if d == "time" else d for d in rdims)
    coords = {k: v for k, v in coords.items() if k != "time"}
    coords["period"] = labels
    data = dict(zip(variables, res)) if powers is not None else {variables: res}
    return _agg._as_dataset(data, rdims, coords, was_xr)


def _check_cells(cells, route=None):
    """``cells=`` of the period calls: "all" or "referenced"; the latter sums the field first, so it excludes ``_route="aggregate_first"``"""
    if cells not in ("all", "referenced"):
        raise ValueError("cells must be 'all' or 'referenced', got %r" % (cells,))
    if cells == "referenced" and route == "aggregate_first":
        raise ValueError("cells='referenced' sums the field first: it cannot be combined with _route='aggregate_first'")


def _reduce_first_possible(ds, variable, powers):
    if not (isinstance(ds, _agg.ReindexedDataset) and variable in ds._src_values):
        return False
    dims = ds._src_dims[variable]
    *_, others = _spatial_layout(dims)
    return [dims[i] for i in others] == ["time"] and _flatten_for_device_layout(dims) == "TG"


def _flatten_for_device_layout(dims):
    """The layout _flatten_for_device gives these dims ("GT" only for (lat, lon, ...) / (lon, lat, ...))."""
    _, _, first, second, others = _spatial_layout(dims)
    return "GT" if second == first + 1 and others and all(i > second for i in others) else "TG"


def weighted_aggregate_grid_to_regions_periods(ds, variable, aggwt, agglev, weights, period="year", backup_aggwt="areawt",
                                               _route=None, season=None, cells="all"):
    """``weighted_aggregate_grid_to_regions`` followed by the sum over each period's time steps, all on the device.

    ds, variable, aggwt, agglev, weights   as for :func:`weighted_aggregate_grid_to_regions` (``weights``: the segment table,
              a :class:`PreparedWeights`, or the path of the CSV)
    period    "year" (one period per calendar year), "month" (one per year-month, labelled ``year * 100 + month``) or a
              length-T array of labels (equal labels form a period; a negative integer or ``None`` drops the row); periods
              come out in ascending label order.  ``time`` may be datetime64 or the YYYYDDD integers of ``tas_poly``; on
              datetime64 time 29 February is summed like any day (``tas_poly`` has removed it from its own variables).
              Anything else raises ValueError (:func:`period_rows`).
    backup_aggwt   the weights column that stands in wherever ``aggwt`` is not > 0
    season    None, or a growing-season mask: what :func:`climate_toolbox_amd.seasons.get_daily_growing_season_mask` or
              :func:`~climate_toolbox_amd.seasons.season_windows` returned.  Only the days on which a cell is in season count
              for it -- the total of ``mask * field`` aggregated daily, with a day out of season counting 0 like a NaN term
              (its weight stays in the denominator).  The mask's grid is joined to the dataset's ``lat`` / ``lon`` by exact
              label equality (KeyError for a dataset cell the mask lacks); the days are those of the dataset's own ``time``.
              One route whatever the plan: the field is summed per period first (``wagg_season_reduce_*``), P rows are
              contracted.  A (lat, lon, time) field is transposed on the device; a host-resident field is uploaded WHOLE --
              this route does not use the quads-only host pipeline of the daily call.  A further non-time dimension, an
              in-season +-inf (there is no daily masked route to fall back to) or ``_route=`` with it raise ValueError.
    cells     "all" (the default: everything above, unchanged) or "referenced": the field is first PACKED to the 16-byte quads
              the segment table references (``engine.pack_rows``: a third of a c2-real row) -- by host threads for a
              host-resident field, so that only those quads cross PCIe (where the library takes that way: a field of >= 64 MiB,
              enough CPUs; else it is uploaded whole and packed on the device), by one kernel for a device-resident one -- then
              summed per period over Gq cells instead of G and contracted through the plan's quads-only cell table.  It always
              sums the field first (with ``_route="aggregate_first"`` ValueError), with or without ``season=``.  Results agree
              with "all" to the rounding of the fp64 partial sums.  One difference: a +-inf in a cell of a quad no table row
              reads is no longer seen -- it neither raises (``season=``) nor sends the call down the daily route.  Where the
              plan has no quads map (a dense-family plan, a grid the whole-line chunkings do not serve) or the packed row
              exceeds 80 % of the row, the call runs as with "all": the keyword permits, it never fails.

    Returns the single call's Dataset with ``time`` replaced by a dimension ``period`` carrying the labels; region labels,
    other coordinates and the variable name are unchanged.  Lazy variables (``tas_poly``, ``convert_kelvin_to_celsius``,
    ``snyder_edd``, ``snyder_gdd``) are evaluated per cell and day before anything is summed; ``results_on_device()`` is
    honoured as in the single call.

    Semantics: the result equals the sum over each period's rows of the daily result.  A NaN daily value -- a region whose
    denominator is zero -- makes the period NaN: a plain sum does not skip NaN.

    Dense-family plans on device-resident (time, gridcell) data sum the field first and contract P rows; everything else
    aggregates daily and sums the (T x R) result on the device (``REDUCE_FIRST_FAMILIES``; the module docstring)."""
    if season is not None and _route is not None:
        raise ValueError("_route cannot be combined with season=: season totals always sum the field first")
    _check_cells(cells, _route)
    if weights is None:
        weights = _agg.prepare_spatial_weights_data()         # TypeError, like the reference
    elif isinstance(weights, str):
        weights = _agg.prepare_spatial_weights_data(weights)
    if "time" not in ds.coords:
        raise ValueError("the dataset has no 'time' coordinate to form periods from")
    time_values = np.asarray(ds.coords["time"].values)
    grid = None if season is None else (np.asarray(ds.coords["lat"].values), np.asarray(ds.coords["lon"].values))
    re = _agg._reindex_spatial_data_to_regions(ds, weights)
    return _aggregate_periods(re, variable, aggwt, agglev, weights, backup_aggwt, period, time_values, route=_route, season=season,
                              grid=grid, cells=cells)
