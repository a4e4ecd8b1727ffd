"""``cells=`` of the period calls and the packed-row binding, as far as they go without a GPU: argument checks that run before any
device work, the fallback rule of ``cells="referenced"``, and the C-ABI's new names (tests/test_gpu_packed_totals.py has the rest)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny():
    import pandas as pd
    from climate_toolbox_amd import minixr
    lat, lon = np.arange(4) * 0.5, np.arange(8) * 0.5
    ds = minixr.Dataset({k: (("time", "lat", "lon"), np.ones((3, 4, 8), dtype=np.float32)) for k in ("tas", "tasmin", "tasmax")},
                        coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": lat, "lon": lon})
    for k in ("tasmin", "tasmax"):
        ds[k].attrs["units"] = "C"
    df = pd.DataFrame({"lat": [0.0], "lon": [0.0], "areawt": [1.0], "popwt": [1.0], "reg": [0]})
    return ds, df


def test_bad_cells_arguments_raise_before_any_device_work():
    """an unknown ``cells``, "referenced" with ``_route="aggregate_first"`` (it sums the field first) and "referenced" without a
    period are ValueError in all three public calls"""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd.transformations import snyder_edd_aggregate, tas_poly_aggregate
    ds, df = _tiny()
    agg = pkg.weighted_aggregate_grid_to_regions_periods
    with pytest.raises(ValueError, match="cells must be"):
        agg(ds, "tas", "popwt", "reg", df, cells="some")
    with pytest.raises(ValueError, match="aggregate_first"):
        agg(ds, "tas", "popwt", "reg", df, cells="referenced", _route="aggregate_first")
    with pytest.raises(ValueError, match="cells must be"):
        tas_poly_aggregate(ds, [1], "popwt", "reg", df, period="year", cells=None)
    with pytest.raises(ValueError, match="aggregate_first"):
        tas_poly_aggregate(ds, [1], "popwt", "reg", df, period="year", cells="referenced", _route="aggregate_first")
    with pytest.raises(ValueError, match="needs period"):
        tas_poly_aggregate(ds, [1], "popwt", "reg", df, cells="referenced")
    with pytest.raises(ValueError, match="cells must be"):
        snyder_edd_aggregate(ds, [10.0], "popwt", "reg", df, period="year", cells="quads")
    with pytest.raises(ValueError, match="needs period"):
        snyder_edd_aggregate(ds, [10.0], "popwt", "reg", df, cells="referenced")


def test_the_default_is_all_cells():
    import inspect
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import periods, seasons
    from climate_toolbox_amd.transformations import snyder_edd_aggregate, tas_poly_aggregate
    for fn in (pkg.weighted_aggregate_grid_to_regions_periods, tas_poly_aggregate, snyder_edd_aggregate, periods._aggregate_periods,
               periods._reduce_first, seasons._season_totals, seasons._ladder_totals):
        assert inspect.signature(fn).parameters["cells"].default == "all", fn.__name__


def _stub_plan(G, cells_by_elem):
    from climate_toolbox_amd import engine
    plan = engine.SparsePlan.__new__(engine.SparsePlan)          # (no device: the cache of compact_cells stands in for the library)
    plan.G, plan._compact_cells, plan._h = G, dict(cells_by_elem), C.c_void_p()
    return plan


def test_referenced_falls_back_where_the_plan_cannot_pack():
    """seasons._compact_cells_of: None -- the call runs as with cells="all" -- for a dense-family plan, a plan without the quads
    map for the element type, and a packed row above 80 % of the row (5 Gq > 4 G); the cells otherwise"""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.seasons import _compact_cells_of
    dense = engine.DensePlan.__new__(engine.DensePlan)
    dense._h = None
    assert _compact_cells_of(dense, np.float32) is None
    assert _compact_cells_of(object(), np.float32) is None
    G = 40
    cells32 = np.arange(32, dtype=np.int32)                      # 32 of 40 cells: exactly 80 %
    plan = _stub_plan(G, {4: cells32, 8: None})
    assert _compact_cells_of(plan, np.float32) is cells32
    assert _compact_cells_of(plan, "torch.float32") is cells32
    assert _compact_cells_of(plan, np.float64) is None           # no map for fp64 data
    assert _compact_cells_of(_stub_plan(G, {4: np.arange(36, dtype=np.int32)}), np.float32) is None      # 90 % of the row


def test_pack_stats_and_flag_values():
    from climate_toolbox_amd import _lib, engine
    assert set(engine.PACK_STATS) == {"device", "host", "host_fallback"}
    assert all(isinstance(v, int) for v in engine.PACK_STATS.values())
    text = open(os.path.join(ROOT, "include", "wagg.h")).read()
    assert int(re.search(r"#define WAGG_APPLY_COMPACT_ROWS (0x[0-9a-fA-F]+)", text).group(1), 16) == _lib.APPLY_COMPACT_ROWS
    assert _lib.APPLY_COMPACT_ROWS & (_lib.APPLY_EXACT_F32 | _lib.HOST_PIN | _lib.HOST_WHOLE | _lib.HOST_LINES | _lib.HOST_LINES_WHOLE) == 0
    for name in ("wagg_plan_compact_info", "wagg_plan_compact_cells", "wagg_pack_rows_f32", "wagg_pack_rows_f64",
                 "wagg_pack_rows_host_f32", "wagg_pack_rows_host_f64"):
        assert name in _lib.EXPORTS and re.search(r"\bint %s\(" % name, text), name


def test_the_library_exports_the_new_names_and_checks_their_arguments():
    """no device needed: NULL arguments and a bad element size are WAGG_EINVAL; the descriptor did not grow"""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    gq = C.c_int64(7)
    assert L.wagg_plan_compact_info(None, 4, C.byref(gq)) == -1
    assert L.wagg_plan_compact_cells(None, 4, None) == -1
    assert L.wagg_pack_rows_f32(None, None, None, 1, 1, None, 1, None) == -1
    assert L.wagg_pack_rows_host_f64(None, None, None, 1, 1, None, 1, 0) == -1
    assert L.wagg_struct_size(_lib.STRUCT_APPLY_DESC) == C.sizeof(_lib.ApplyDesc) == 176
    assert L.wagg_struct_size(_lib.STRUCT_HOST_STATS) == C.sizeof(_lib.HostStats) == 18 * 8
    assert L.wagg_version() >= 900
