"""Several aggregations of one field from one pass: ``weighted_aggregate_grid_to_regions_many`` over many-plans
(``engine.ManyPlan``, ``wagg_plan_create_many``), and the helpers that decide which requested levels are derived from a
finer one."""
from __future__ import annotations

import numpy as np

from . import aggregations as _A
from ._lib import HOST_LINES, HOST_PIN
from ._plans import _many_plan_for
from .engine import require_gpu

MAX_WEIGHTS = 4          # wagg.h: weightings per many-plan


def nest_map(fine_code, coarse_code, kept=None):
    """fine -> coarse code map if the coarse level nests in the fine one, else None.

    Per-row integer codes (< 0 = null label).  Over the rows of ``kept`` (a boolean mask; None = every row) -- the rule of
    wagg_plan_create_many, which checks the rows some weighting keeps -- the fine code is null exactly where the coarse one
    is and each fine code meets a single coarse code.  The map has one entry per fine code (max + 1 of them); -1 marks a
    fine code no checked row uses."""
    f = np.asarray(fine_code, dtype=np.int64)
    c = np.asarray(coarse_code, dtype=np.int64)
    if f.shape != c.shape or f.ndim != 1:
        raise ValueError("fine_code and coarse_code must be 1-D and of equal length")
    if kept is not None:
        f, c = f[np.asarray(kept, dtype=bool)], c[np.asarray(kept, dtype=bool)]
    fn, cn = f < 0, c < 0
    if (fn != cn).any():
        return None
    f, c = f[~fn], c[~fn]
    m = np.full(int(f.max()) + 1 if len(f) else 0, -1, dtype=np.int64)
    m[f] = c
    return m if (m[f] == c).all() else None


def nesting_order(codes, kept=None):
    """Group requested levels for many-plans: ``codes`` maps a level name to its per-row codes (same rows).  Returns
    ``[(base, [derived, ...]), ...]``: each base level with the levels that nest in it (over ``kept``), the finest first.
    A level that nests in no other requested level is a base of its own."""
    names = list(codes)
    nreg = {n: int(np.asarray(codes[n]).max()) + 1 if len(codes[n]) else 0 for n in names}
    groups, placed = [], set()
    for base in sorted(names, key=lambda n: -nreg[n]):
        if base in placed:
            continue
        placed.add(base)
        derived = [n for n in names if n not in placed and nest_map(codes[base], codes[n], kept) is not None]
        placed.update(derived)
        groups.append((base, derived))
    return groups


def _single(ds, variable, combos, weights, backup_aggwt):
    out = {}
    for aggwt, agglev in combos:
        rds = _A._reindex_spatial_data_to_regions(ds, weights)
        out[(aggwt, agglev)] = _A._aggregate_reindexed_data_to_regions(rds, variable, aggwt, agglev, weights, backup_aggwt)
    return out


def weighted_aggregate_grid_to_regions_many(ds, variable, combos, weights, backup_aggwt="areawt"):
    """Several ``weighted_aggregate_grid_to_regions(ds, variable, aggwt, agglev, weights)`` at once, e.g.
    ``combos = [("popwt", "hierid"), ("areawt", "hierid"), ("popwt", "ISO"), ("areawt", "ISO")]``.

    Returns ``{(aggwt, agglev): Dataset}``, each with the names, dims, coords and labels of the single call.  The field is
    reindexed once and every level factorised once; the weightings of a level share one pass over X (one PCIe crossing for a
    host-resident field), and a level that nests in a finer requested one is derived from that level's partial sums.  Levels
    that nest in none get a many-plan of their own.  Routing is the single call's: a host-resident (time, gridcell) field
    goes through the row-block pipeline (``HOST_PIN | HOST_LINES``), a device-resident one stays on the device, and
    ``results_on_device()`` is honoured.  Lazily transformed variables (``tas_poly``, ``snyder_*``), already materialised
    datasets and tables the dense family serves take the single calls, which give the same results by construction."""
    combos = [(str(a), str(b)) for a, b in combos]
    if isinstance(weights, str):
        weights = _A.prepare_spatial_weights_data(weights)
    if not combos:
        return {}
    rds = _A._reindex_spatial_data_to_regions(ds, weights)                       # once
    if (not isinstance(rds, _A.ReindexedDataset) or variable not in rds._src_values or rds._xforms.get(variable) is not None
            or rds._edds.get(variable) is not None):
        return _single(ds, variable, combos, weights, backup_aggwt)
    values, dims = rds._src_values[variable], rds._src_dims[variable]
    cell_idx, G = rds._cell_index(variable)
    if len(cell_idx) != len(weights):
        raise ValueError("weights has %d rows but the dataset was reindexed with %d" % (len(weights), len(cell_idx)))
    shape = dict(zip(dims, tuple(values.shape)))
    ia, io, *_ = _A._spatial_layout(dims)
    row_len = shape["lon"] if ia < io else shape["lat"]
    require_gpu()
    X2, layout, _, unflatten = _A._flatten_for_device(values, dims)
    is_f32 = str(X2.dtype).endswith("float32")
    on_dev = _A._is_device_tensor(X2)
    keep_dev = _A._device_results_wanted() and on_dev and not rds._was_xarray
    carried = dict(rds.coords)

    aggwts = list(dict.fromkeys(a for a, _ in combos))
    w_eff = {a: _A._backup_fill(weights[a].values, weights[backup_aggwt].values) for a in aggwts}      # once per weighting
    fact = {lv: _A._factorize_labels(np.asarray(weights[lv].values)) for lv in dict.fromkeys(b for _, b in combos)}  # once per level
    kept = np.zeros(len(cell_idx), dtype=bool)
    for a in aggwts:
        kept |= ~np.isnan(w_eff[a])
    # derived levels need the whole-line chunking: (time, gridcell) data of a grid with a row length
    if layout == "TG" and row_len > 0:
        groups = nesting_order({lv: codes for lv, (_u, codes) in fact.items()}, kept)
    else:
        groups = [(lv, []) for lv in fact]
    out_layout = "TR" if layout == "TG" else "RT"
    Xd = None
    results, leftover = {}, []

    def dataset(plane, agglev):
        uniq = fact[agglev][0]
        res = unflatten(plane if keep_dev else (np.ascontiguousarray(plane) if isinstance(plane, np.ndarray) else _A._to_host(plane.contiguous())),
                        len(uniq))
        rdims = _A._result_dims(dims, agglev)
        coords = {d: np.asarray(carried[d].values) for d in rdims if d != agglev and d in carried and tuple(carried[d].dims) == (d,)}
        coords[agglev] = uniq
        return _A._as_dataset({variable: res}, rdims, coords, rds._was_xarray)

    while groups:
        base, derived = groups.pop(0)
        levels = [base] + derived
        wanted = [a for a in aggwts if any((a, lv) in combos for lv in levels)]
        for k0 in range(0, len(wanted), MAX_WEIGHTS):
            ws = wanted[k0:k0 + MAX_WEIGHTS]
            ub, cb = fact[base]
            plan = _many_plan_for(cell_idx, cb, [w_eff[a] for a in ws], G, len(ub), row_len,
                                  [(fact[lv][1], len(fact[lv][0])) for lv in derived], is_f32=is_f32, layout=layout)
            if plan is None:                                                # the dense family serves this table
                leftover += [(a, lv) for a in ws for lv in levels if (a, lv) in combos]
                continue
            try:
                if derived and not (plan.info["lines"] & (1 if is_f32 else 2)):
                    groups += [(lv, []) for lv in levels]                   # no whole-line chunking: each level on its own
                    break
                if not on_dev and layout == "TG":
                    X2c = np.ascontiguousarray(X2)
                    views = plan.apply_host(X2c, flags=HOST_PIN | HOST_LINES)
                else:
                    if Xd is None:
                        Xd = _A._to_device(X2)
                    views = plan.apply(Xd, layout=layout, out_layout=out_layout)
                    if not keep_dev:
                        plan.status()                               # a device-side failure must not pass silently
                    else:                                           # (inside results_on_device(): checked when the block ends)
                        pending = getattr(_A._TLS, "unchecked_plans", None)
                        if pending is not None and not any(p is plan for p in pending):
                            pending.append(plan)
                for li, lv in enumerate(levels):
                    for ki, a in enumerate(ws):
                        if (a, lv) in combos:
                            results[(a, lv)] = dataset(views[li][ki], lv)
            except _A.WaggError:
                _A._drop_plan(plan)
                raise
            finally:
                plan._lease.release()
    if leftover:
        results.update(_single(ds, variable, leftover, weights, backup_aggwt))
    return {c: results[c] for c in combos}
