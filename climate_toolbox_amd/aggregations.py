"""Drop-in for ``climate_toolbox.aggregations.aggregations`` -- same names, arguments and error
behaviour; the arithmetic runs on MI355X through libwagg.so (include/wagg.h).

Reference (read as text): /root/reference/climate_toolbox/aggregations/aggregations.py
  _reindex_spatial_data_to_regions       :8-32     -> here: label lookup on host, NO data copy
  _aggregate_reindexed_data_to_regions   :35-84    -> here: backup fill + label factorisation on
                                                      host (fp64), grouped sums + division on GPU
  weighted_aggregate_grid_to_regions     :87-124
  prepare_spatial_weights_data           :127-152

What stays on the host (before the C-ABI), exactly as SURVEY.md section 8b lays out: exact float
label matching (S1), the per-row backup fill (S4), sorted-unique label factorisation (S3).  What
the GPU does: the gather of :27 fused into the weighted group sums of :78-79 and the division.
There is no CPU compute path: without the HIP library or a GPU these functions raise.

This module holds the four reference names, the shared aggregation body and the two switches of the drop-in
(``HOST_DEVICES``, ``results_on_device``).  What they stand on lives beside it (round 6) and is re-exported here, so
``aggregations.X`` resolves as before:
  _memo.py       table fingerprints, the per-table memo, the caches' lock
  _labels.py     exact label join, backup fill, label factorisation (native, memoised)
  _layout.py     (..., lat, lon, ...) <-> (time x gridcell) bookkeeping
  _reindexed.py  the lazy ReindexedDataset and the Dataset accessors
  _pinned.py     the page-locked result pool
  _plans.py      family choice, the leased plan cache, replicas
  _prepared.py   PreparedWeights / prepare_weights
"""
from __future__ import annotations

import functools
import threading

import numpy as np
import pandas as pd

from . import _labels, _lib as _libmod, _pinned, _plans, engine as _engine, minixr
from ._labels import (_backup_fill, _exact_index, _factorize_labels, _factorize_labels_impl, _is_null_label, _native,  # noqa: F401
                      _resolve_cells, _resolve_cells_impl)
from ._layout import _flatten_for_device, _is_device_tensor, _result_dims, _spatial_layout, _to_device  # noqa: F401
from ._lib import FORM_ENTRIES, WaggError  # noqa: F401
from ._memo import (_CACHE_LOCK, _POINTER_TABLES, _TABLE_MEMO, _TABLE_MEMO_MAX, _Unhashable, _f64, _fingerprint, _frozen,  # noqa: F401
                    _clear_memos, _memo, _raw_view)
from ._pinned import _PINNED_POOL, _pinned_result, _to_host  # noqa: F401
from ._plans import (DENSE_SWITCH, _PLAN_CACHE, _dense_bytes, _drop_plan, _evict_plans, _host_quantum, _plan_bytes, _plan_for,  # noqa: F401
                     _prefer_dense, _wants_dense)
from ._prepared import PreparedWeights, prepare_weights
from ._reindexed import ReindexedDataset, _edds, _extract, _is_xarray, _lon_perms, _ReindexedArray, _xforms, _xr  # noqa: F401
from .engine import DensePlan, SparsePlan, require_gpu

__all__ = ["weighted_aggregate_grid_to_regions", "prepare_spatial_weights_data", "prepare_weights", "PreparedWeights", "clear_caches",
           "_reindex_spatial_data_to_regions", "_aggregate_reindexed_data_to_regions"]


# Host-resident fields stream through the CURRENT device only by default.  Several row-block pipelines from one process
# (one per device, each on its own PCIe link; SURVEY 8b `n_devices`, 8e "one process driving all devices") are an explicit
# opt-in: HOST_DEVICES = "all" (every visible device -- never inside a one-process-per-GPU job, where every rank sees all
# devices: such processes, recognised by WORLD_SIZE > 1 in the environment, stay on their own device) or a list of device
# ordinals (a device may be listed twice: two pipelines on one GPU).  The multi-device form has only ever run with several
# pipelines on ONE physical device (gpurun exposes one GPU), hence the conservative default.
HOST_DEVICES = None


def _host_devices():
    return _plans._host_devices(HOST_DEVICES)


def _host_replicas(plan, n_rows, row_bytes):
    return _plans._host_replicas(plan, n_rows, row_bytes, HOST_DEVICES)


_TLS = threading.local()


class results_on_device:
    """``with climate_toolbox_amd.results_on_device(): out = weighted_aggregate_grid_to_regions(ds, ...)`` -- for a variable
    whose buffer is a torch CUDA tensor the returned Dataset's variable is a torch CUDA tensor too (same device, queued on
    the current stream; the call does not wait for it).  A loop over variables that feeds further GPU work then pays the
    kernels only; everything else about the call -- names, dims, the ``agglev`` coordinate, the numbers -- is unchanged
    (bit-equal to the host route).  Per thread; nests; host-resident variables and xarray Datasets still return host arrays.
    The reference has no such switch (it computes on the host, aggregations.py:75-82): this is an extension.

    Failures stay visible: a call inside the block does not wait for its kernels, so it cannot report a device-side failure
    of its segment-table plan itself; the plans such calls used are remembered and checked (``wagg_plan_status``: one stream
    synchronisation per plan) when the OUTERMOST block ends, and a failed one raises there -- before the caller's code
    behind the block consumes the tensors -- and is dropped from the cache.  (No kernel of libwagg.so can fail that way;
    the diagnostic build's bounded-spin kernel can.)"""

    def __init__(self, on=True):
        self._on = bool(on)

    def __enter__(self):
        self._prev = getattr(_TLS, "device_results", False)
        self._outermost = not hasattr(_TLS, "unchecked_plans")
        if self._outermost:
            _TLS.unchecked_plans = []
        _TLS.device_results = self._on
        return self

    def __exit__(self, *exc):
        _TLS.device_results = self._prev
        if self._outermost:
            plans = _TLS.unchecked_plans
            del _TLS.unchecked_plans
            if exc[0] is None:
                for plan in plans:
                    if getattr(plan, "_h", None) is not None and plan._h.value:       # (a plan evicted meanwhile has been drained by close)
                        try:
                            plan.status()
                        except WaggError:
                            _drop_plan(plan)
                            raise
        return False


def _device_results_wanted():
    return getattr(_TLS, "device_results", False)


def clear_caches():
    """Give back what the package keeps between calls: cached plans that no call is using (device memory), the table memos,
    the coded tables of the CSV route, the FREE blocks of the page-locked result pool (blocks behind results the caller
    still holds return to the pool when those are dropped, and go with the next call of this function) and the device
    scratch the library keeps from one plan build to the next (``wagg_release_scratch``)."""
    _plans._clear_plans()
    _clear_memos()
    with _CACHE_LOCK:
        _PREPARED_BY_PATH.clear()
    _pinned._clear_free_blocks()
    if _libmod._lib is not None:
        _libmod._lib.wagg_release_scratch()


_PREPARED_BY_PATH = {}      # (path, aggwt, agglev) -> PreparedWeights: the CSV route is memoised on the path like the reference (:127)


# ----------------------------------------------------------------------------------------------
# the reference's functions
# ----------------------------------------------------------------------------------------------
def _reindex_spatial_data_to_regions(ds, df):
    """Drop-in for aggregations.py:8-32.

    Every row ``i`` of the segment table ``df`` selects the grid cell whose labels equal
    ``df.lat[i]`` / ``df.lon[i]`` exactly (``KeyError`` when a label is not on the grid); the new
    ``reshape_index`` dimension takes the place of the first of the two indexed dims.  What comes
    back is a lazy :class:`ReindexedDataset`: the cell index of every row, no gathered copy.
    """
    src_values, src_dims, coords, was_xr = _extract(ds)
    if "lat" not in coords or "lon" not in coords:
        raise KeyError("dataset must have 'lat' and 'lon' coordinates (aggregations.py:27)")
    lat = np.asarray(coords["lat"].values)
    lon = np.asarray(coords["lon"].values)
    prepared = df if isinstance(df, PreparedWeights) else None
    if prepared is not None:
        cell, ilat, ilon = prepared.cells_for(lat, lon)                          # resolved once per grid
        seg_lat, seg_lon = prepared.seg_lat, prepared.seg_lon
    else:
        seg_lat, seg_lon = df["lat"].values, df["lon"].values
        cell = _resolve_cells(lat, lon, seg_lat, seg_lon)                        # native, KeyError on a miss
        ilat, ilon = (cell // len(lon)).astype(np.int64), (cell % len(lon)).astype(np.int64)
    # xarray's vectorised sel indexes EVERY data variable (S9); variables without lat/lon dims
    # are carried through untouched
    keep_vals, keep_dims = {}, {}
    passthrough = {}
    for k, dims in src_dims.items():
        if "lat" in dims and "lon" in dims:
            keep_vals[k], keep_dims[k] = src_values[k], dims
        else:
            passthrough[k] = minixr.DataArray(src_values[k], dims)
    out = ReindexedDataset(keep_vals, keep_dims, coords, ilat, ilon, seg_lat, seg_lon,
                           was_xr, lon_perms=_lon_perms(ds), xforms=_xforms(ds), edds=_edds(ds))
    if prepared is not None:
        out._row_major_cell = (cell, len(lat), len(lon))                         # = ilat * nlon + ilon, already int32
    for k, v in passthrough.items():
        out.data_vars[k] = v
    return out


def _aggregate_core(ds, variable, aggwt, agglev, weights, backup_aggwt, powers=None, offset=0.0, edd_planes=False):
    """Shared body of the aggregation.  ``powers=None``: aggregate ``variable`` as it is (with its
    own lazy transform, if it carries one).  ``powers=[p, ...]``: aggregate ``(x + offset) ** p``
    for every p in ONE pass over the data.  ``edd_planes``: a degree-day variable's thresholds come back one
    result each (a list) instead of combined.  Returns (list of result arrays, result dims, coords, was_xarray)."""
    prepared = weights if isinstance(weights, PreparedWeights) else None
    if prepared is not None:
        prepared.check(aggwt, agglev, backup_aggwt)
        w_eff, labels, uniq, codes = prepared.w_eff, prepared.labels, prepared.uniq.copy(), prepared.codes
    else:
        w_eff = _backup_fill(weights[aggwt].values, weights[backup_aggwt].values)   # :73 (native)
        labels = np.asarray(weights[agglev].values)
        uniq, codes = _factorize_labels(labels)                          # :78 group keys

    xform = edd = None
    if isinstance(ds, ReindexedDataset) and variable in ds._src_values:
        values, dims = ds._src_values[variable], ds._src_dims[variable]
        xform = ds._xforms.get(variable)
        edd = ds._edds.get(variable)
        cell_idx, G = ds._cell_index(variable)
        if len(cell_idx) != len(w_eff):
            raise ValueError("weights has %d rows but the dataset was reindexed with %d"
                             % (len(w_eff), len(cell_idx)))
        shape = dict(zip(dims, tuple(values.shape)))
        ia, io, *_ = _spatial_layout(dims)
        row_len = shape["lon"] if ia < io else shape["lat"]
        was_xr = ds._was_xarray
        carried = {k: v for k, v in ds.coords.items()}
        # mirror the mutation of :64-71
        ds.coords[agglev] = minixr.DataArray(labels, ("reshape_index",))
        ds.data_vars[aggwt] = minixr.DataArray(w_eff, ("reshape_index",), name=aggwt)
    else:
        # an already materialised dataset: its reshape_index axis is the "grid"
        arr = ds[variable]
        dims = tuple(arr.dims)
        if "reshape_index" not in dims:
            raise KeyError("dataset has no 'reshape_index' dimension; call "
                           "_reindex_spatial_data_to_regions first")
        values = np.asarray(arr.values)
        k = dims.index("reshape_index")
        # present it as (lat=reshape_index, lon=1) so that the same flattening code applies
        dims = dims[:k] + ("lat", "lon") + dims[k + 1:]
        values = values.reshape(values.shape[:k] + (values.shape[k], 1) + values.shape[k + 1:])
        G = values.shape[k]
        cell_idx = np.arange(G, dtype=np.int32)
        if G != len(w_eff):
            raise ValueError("weights has %d rows but reshape_index has %d" % (len(w_eff), G))
        row_len = 0
        was_xr = _is_xarray(ds)
        carried = ({k2: minixr.DataArray(v.values, tuple(v.dims)) for k2, v in ds.coords.items()}
                   if was_xr else dict(ds.coords))

    if (powers is not None or edd is not None) and xform is not None:
        raise ValueError("variable %r already carries a lazy transform" % (variable,))
    if powers is None and xform is not None:
        offset, powers, single = xform[0], [xform[1]], True
    else:
        single = powers is None
    torch = require_gpu()
    X2, layout, _, unflatten = _flatten_for_device(values, dims)
    is_f32 = str(X2.dtype).endswith("float32")

    def result_coords():
        """dims of the result (S10) and its coordinates: the carried 1-D coords plus the sorted unique labels (S3)"""
        rdims = _result_dims(dims, agglev)
        coords = {d: np.asarray(carried[d].values) for d in rdims if d != agglev and d in carried and tuple(carried[d].dims) == (d,)}
        coords[agglev] = uniq
        return rdims, coords

    def _aggregate_on_plan(plan):
        out_layout = "TR" if layout == "TG" else "RT"
        if (not _is_device_tensor(X2)) and layout == "TG" and powers is None and edd is None:
            # Host-resident (time, gridcell) field, plain aggregation: the C-ABI streams it through the device
            # in row blocks, the arrays page-locked in place for the call (wagg_apply_host_ex_* /
            # wagg_dense_apply_host_*): the H2D of block i+1 overlaps the kernels of block i and the device
            # never holds the whole field.  PCIe-bound for the segment-table form (49 GB/s of X, ~100x the
            # kernel), 13 % faster than copy-then-compute for a dense 1,369-row shard (tools/host_path_timing.py).
            from ._lib import HOST_LINES, HOST_PIN
            X2c = np.ascontiguousarray(X2)
            # (the result lands in a page-locked block of the result pool: nothing to register, no first-touch page faults)
            host_out = plan.apply_host(X2c, flags=HOST_PIN | HOST_LINES, replicas=_host_replicas(plan, X2c.shape[0], X2c.strides[0]),
                                       out=_pinned_result((X2c.shape[0], plan.R), X2c.dtype))
            if isinstance(plan, DensePlan) and plan.saw_inf():       # +-inf: redo in the exact segment-table form (S6)
                exact = SparsePlan(cell_idx, codes, w_eff, G, len(uniq), row_len=row_len)
                try:
                    host_out = exact.apply_host(X2c, flags=HOST_PIN)
                finally:
                    exact.close()
            res0 = unflatten(host_out, len(uniq))
            rdims, coords = result_coords()
            return res0, rdims, coords, was_xr
        if ((not _is_device_tensor(X2)) and layout == "TG" and powers is not None and edd is None and isinstance(plan, SparsePlan)
                and max(powers) <= 16 and min(powers) >= 1 and len(_host_devices()) < 2):
            # Host-resident (time, gridcell) field raised to powers (tas_poly, transformations.py:188, then the aggregation):
            # the same row-block pipeline (wagg_apply_poly_host_*) -- the field crosses PCIe once, lines only, and every
            # block is raised to its powers on the device, four per pass.  (Before round 5: one pageable copy of the whole
            # field, ~28 GB/s, then the kernels.)
            from ._lib import HOST_LINES, HOST_PIN
            X2c = np.ascontiguousarray(X2)
            lo, hi = int(min(powers)), int(max(powers))
            stack = plan.apply_poly_host(X2c, offset, hi - lo + 1, pow_first=lo, flags=HOST_PIN | HOST_LINES,
                                         out=_pinned_result((hi - lo + 1, X2c.shape[0], plan.R), X2c.dtype))
            res = [unflatten(stack[int(p) - lo], len(uniq)) for p in powers]
            rdims, coords = result_coords()
            return (res[0] if single else res), rdims, coords, was_xr
        if ((not _is_device_tensor(X2)) and layout == "TG" and edd is not None and isinstance(plan, SparsePlan)
                and len(edd[2]) == 1 and edd[2][0][0] == 1.0 and len(_host_devices()) < 2 and not edd_planes):
            # Host-resident tasmin / tasmax, one set of degree days (snyder_edd, transformations.py:7-93, then the aggregation):
            # both fields through the row-block pipeline together (wagg_apply_edd_host_*), lines only.  (A combination of
            # several degree-day planes -- snyder_gdd -- is summed on the device: the upload-then-kernels way below.)
            H2 = _flatten_for_device(edd[0], dims)[0]
            if not _is_device_tensor(H2):
                if H2.shape != X2.shape or H2.dtype != X2.dtype:
                    raise ValueError("tasmin and tasmax must have the same shape and dtype")
                from ._lib import HOST_LINES, HOST_PIN
                stack = plan.apply_edd_host(np.ascontiguousarray(X2), np.ascontiguousarray(H2), [edd[2][0][1]], offset=edd[1],
                                            flags=HOST_PIN | HOST_LINES, out=_pinned_result((1, X2.shape[0], plan.R), X2.dtype))
                rdims, coords = result_coords()
                return unflatten(stack[0], len(uniq)), rdims, coords, was_xr
        # everything else: one pageable H2D copy of the field (fields already on the device pass through), the
        # kernels, one D2H copy of the result
        Xd = _to_device(X2)
        if edd is not None:
            # Snyder degree days: sum of coef * EDD(threshold), both fields loaded once per threshold
            H2 = _flatten_for_device(edd[0], dims)[0]
            if H2.shape != X2.shape or H2.dtype != X2.dtype:
                raise ValueError("tasmin and tasmax must have the same shape and dtype")
            Hd = _to_device(H2)
            coefs, thr = [c for c, _ in edd[2]], [e for _, e in edd[2]]

        def run(plan):
            """The device work for one plan form; returns the list of (T, R) / (R, T) result tensors."""
            if edd is not None:
                if isinstance(plan, DensePlan):     # the degree days are evaluated while X is packed, one threshold per apply
                    stack = torch.empty((len(thr), Xd.shape[0], plan.R), dtype=Xd.dtype, device=Xd.device)
                    for k, e in enumerate(thr):
                        plan.apply_edd(Xd, Hd, e, offset=edd[1], out=stack[k])
                else:
                    stack = plan.apply_edd(Xd, Hd, thr, offset=edd[1], layout=layout, out_layout=out_layout)
                if edd_planes or (len(coefs) == 1 and coefs[0] == 1.0):
                    return list(stack) if edd_planes else [stack[0]]
                return [_engine.combine_planes(stack, coefs)]     # wagg_combine_planes_*: sum_k coef_k * EDD_k (gdd, :138-140)
            if powers is None:
                return [plan.apply(Xd) if isinstance(plan, DensePlan) else plan.apply(Xd, layout=layout, out_layout=out_layout)]
            if isinstance(plan, DensePlan):         # scattered weights: (x + offset)^p evaluated while X is packed
                return [plan.apply_poly(Xd, offset, int(p)) for p in powers]
            lo, hi = int(min(powers)), int(max(powers))
            stack = plan.apply_poly(Xd, offset, hi - lo + 1, layout=layout, out_layout=out_layout, pow_first=lo)
            return [stack[int(p) - lo] for p in powers]

        outs = run(plan)
        if isinstance(plan, DensePlan) and plan.saw_inf():
            # +-inf in the (transformed) data: the dense forms multiply every (cell, region) pair of a
            # stored tile, so inf * 0 would leak NaN into regions that do not own the cell.  The
            # segment-table form confines it to the owning regions like the reference (S6): redo there.
            exact = SparsePlan(cell_idx, codes, w_eff, G, len(uniq), row_len=row_len)
            try:
                outs = run(exact)
                exact.status()
            finally:
                exact.close()
        # results_on_device(): a device-resident field's result stays a torch CUDA tensor on the caller's stream -- no D2H
        # copy (0.8 of the 1.0 ms of a c2-real call), no wait; the Dataset's variable holds the tensor like minixr holds
        # device buffers on the input side.  (xarray cannot carry one: xarray callers always get host arrays.)
        keep_dev = _device_results_wanted() and _is_device_tensor(X2) and not was_xr
        res = [unflatten(o if keep_dev else _to_host(o), len(uniq)) for o in outs]
        if isinstance(plan, SparsePlan):
            if not keep_dev:
                plan.status()                                    # a device-side failure must not pass silently
            else:                                                # (no wait inside results_on_device(): checked when the block ends)
                pending = getattr(_TLS, "unchecked_plans", None)
                if pending is not None and not any(p is plan for p in pending):
                    pending.append(plan)
        rdims, coords = result_coords()
        return (res if edd_planes else res[0] if single or edd is not None else res), rdims, coords, was_xr

    plan = _plan_for(cell_idx, codes, w_eff, G, len(uniq), row_len, is_f32=is_f32, layout=layout, prepared=prepared)
    try:
        return _aggregate_on_plan(plan)
    except _engine.WaggError:
        # a device-side failure is sticky on the plan (its timeout word): drop it from the cache so the next
        # call on this table builds a fresh one instead of failing for the rest of the process
        _drop_plan(plan)
        raise
    finally:
        plan._lease.release()


def _as_dataset(data_vars, rdims, coords, was_xr):
    if was_xr:
        return _xr.Dataset({k: (rdims, v) for k, v in data_vars.items()}, coords=coords)
    return minixr.Dataset({k: (rdims, v) for k, v in data_vars.items()},
                          coords={k: ((k,), v) for k, v in coords.items()})


def _aggregate_reindexed_data_to_regions(
    ds, variable, aggwt, agglev, weights, backup_aggwt="areawt"
):
    """Drop-in for aggregations.py:35-84: the weighted regional mean of one variable.

    ds            what ``_reindex_spatial_data_to_regions`` returned (or any Dataset that already has
                  a ``reshape_index`` dimension)
    variable      data variable to average
    aggwt         weights column of ``weights`` (popwt, areawt, cropwt, ...)
    agglev        column of ``weights`` holding the region label of each segment row
    weights       the segment table (pandas DataFrame)
    backup_aggwt  column that stands in, row by row, wherever ``aggwt`` is not > 0

    ``w_eff = w if w > 0 else backup`` per ROW (:73, S4); regions are the sorted unique labels
    (:78, S3); ``out = sum(x * w_eff) / sum(w_eff)`` with NaN products counted as 0 (S6) and IEEE
    division (S7).  Like the reference it also attaches ``agglev`` and ``aggwt`` to ``ds`` (:64-71).
    """
    res, rdims, coords, was_xr = _aggregate_core(ds, variable, aggwt, agglev, weights, backup_aggwt)
    return _as_dataset({variable: res}, rdims, coords, was_xr)


def weighted_aggregate_grid_to_regions(ds, variable, aggwt, agglev, weights=None):
    """Drop-in for aggregations.py:87-124: gridded variable -> weighted regional means.

    ds        Dataset (xarray, or minixr here) with ``lat`` and ``lon`` coordinates
    variable  which data variable to aggregate
    aggwt     weighting column of the weights table, e.g. ``popwt`` or ``areawt``
    agglev    region-label column of the weights table, e.g. ``ISO`` or ``hierid``
    weights   the segment-weights DataFrame, or the path of its CSV.  As in the reference
              (:118-119 vs :128) leaving it out cannot work -- no weights file is bundled -- and
              raises TypeError.

    Returns a Dataset holding ``variable`` on ``agglev`` (plus the dims that were carried through).
    """
    if weights is None:
        weights = prepare_spatial_weights_data()          # TypeError, like the reference
    elif isinstance(weights, str):
        # the reference memoises the table on its path (:127): so is its coded form -- a loop over variables that names
        # the file pays for the label work once
        pk = (weights, aggwt, agglev)
        with _CACHE_LOCK:
            prep = _PREPARED_BY_PATH.get(pk)
        if prep is None:
            prep = PreparedWeights(prepare_spatial_weights_data(weights), aggwt, agglev)
            with _CACHE_LOCK:
                _PREPARED_BY_PATH[pk] = prep
        weights = prep

    ds = _reindex_spatial_data_to_regions(ds, weights)
    ds = _aggregate_reindexed_data_to_regions(ds, variable, aggwt, agglev, weights)

    return ds


@functools.lru_cache(maxsize=None)   # the reference memoises on the path (toolz.memoize, :127)
def prepare_spatial_weights_data(weights_file):
    """Drop-in for aggregations.py:127-152: load the segment-weights CSV at ``weights_file``.

    Pixel centres labelled 180.125 are relabelled -179.875 (:144), the index is named
    ``reshape_index`` (:148), ``pix_cent_x/y`` become ``lon/lat`` (:150).  The reference's
    ``drop_duplicates()`` result is discarded (:147), so duplicates are kept here too (they add, S5).
    Memoised like the reference (``toolz.memoize``, :127).
    """
    df = pd.read_csv(weights_file)
    import ctypes as C
    _lib, L = _native()
    x = np.ascontiguousarray(df["pix_cent_x"].values, dtype=np.float64).copy()
    _lib.check(L.wagg_relabel(x.ctypes.data_as(C.POINTER(C.c_double)), len(x), 180.125, -179.875), "wagg_relabel")
    df["pix_cent_x"] = x                                              # aggregations.py:144
    df.index.names = ["reshape_index"]
    df.rename(columns={"pix_cent_x": "lon", "pix_cent_y": "lat"}, inplace=True)
    return df
