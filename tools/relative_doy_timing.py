#!/usr/bin/env python3
"""Spell days against CALENDAR-DAY thresholds, annual totals at c2-real shape (T = 365, 720 x 1440 cells, the synthetic
impact-region table; fp32 and fp64) of a device-resident tasmax-like Kelvin field shifted by ``convert_kelvin_to_celsius``.  The
baseline is ``relative.cell_quantiles(period="calendar_day", window=5)`` over ``--base-years`` years of the same synthetic
variable on the 365-day calendar (30 for fp32: 10950 rows, 365 planes of 150 pooled days -- that build is timed ONCE and recorded
as ``baseline_build``; 10 for fp64, to hold the record in memory); the evaluated year is the record's first.  Cases: q = 0.9 with
``min_length=1`` (TX90p) and ``min_length=6`` (WSDI), and 0.9 / 0.95 / 0.99 with ``min_length=1`` -- with the synthetic 150-day
season windows of tools/season_timing.py ("season") and without ("allyear").  Four arms in one process, alternating inside every
round:

  doy_all          ``tas_relative_spell_aggregate(..., planes="calendar_day", cells="all")``: one launch, the plane picked per row
  doy_referenced   the same with ``cells="referenced"``
  per_threshold    what a user writes today: per level ``hot = x >= thr[k][plane_of_row]`` gathered on the device (and in season),
                   the run-length scan of tools/spell_timing.py, the 0/1 field handed to
                   ``weighted_aggregate_grid_to_regions_periods``: the yardstick
  by_period        for context, not a rival: the by-period call (``planes=None``, ONE annual plane: plane 0 of the baseline) at
                   the same K -- what the per-row threshold reads cost on top of it

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; median, min and max in ms.
No ratio is fixed in advance: the JSON records what was measured, and per case whether a median leads by the project's rule -- by
more than the larger min-max spread of the two arms.  Writes the JSON to the path given as the first argument (default
profiles/relative_doy_timing.json) after every case; ``--only float32`` / ``--only float64`` runs one type.  The synthetic field
has no day-to-day persistence, so runs of six days above a cell's 90th percentile hardly occur: "wsdi6" times the kernel, "tx90p"
carries the agreement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import _lib, engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.relative import CellThresholds, cell_quantiles, resolve_row_planes  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_relative_spell_aggregate  # noqa: E402
from season_timing import growing_days, in_season, measure  # noqa: E402
from spell_timing import leads, run_lengths  # noqa: E402

T, N_TIMED = 365, 12
BASE_YEARS = {"float32": 30, "float64": 10}
CASES = (("tx90p", 1, [0.9]), ("wsdi6", 6, [0.9]), ("tx90p3", 1, [0.9, 0.95, 0.99]))
ARMS = ("doy_all", "doy_referenced", "per_threshold", "by_period")


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    years = dict(BASE_YEARS)
    if "--base-years" in args:
        years = {k: int(args[args.index("--base-years") + 1]) for k in years}
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in ("--only", "--base-years"))]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "relative_doy_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    res = {"T": T, "G": G, "periods": 1, "window": 5, "base_years": years, "group": _lib.CELL_SPELL_GROUP, "timed_calls": N_TIMED,
           "warm_up_s": 0.3,
           "what": "annual days in runs of >= L days at or above each cell's calendar-day percentile (5-day pooled window) of a "
                   "device-resident (365 x G) Kelvin field, aggregated to regions; ms per call, host clock around a device synchronise; "
                   "per_threshold = per level (x >= thr[plane_of_row] gathered, torch run-length scan, "
                   "weighted_aggregate_grid_to_regions_periods); by_period = the same call against ONE plane; leads: the median is "
                   "ahead by more than the larger min-max spread of the two arms"}
    sync = torch.cuda.synchronize

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        Y = years[dtype]
        base_time = np.concatenate([(1981 + y) * 1000 + np.arange(1, 366) for y in range(Y)])
        XB = engine.synth_field(Y * T, G, seed=11, base=297.0, amp=50.0, dtype=dtype).reshape(Y * T, len(lat), len(lon))
        base_ds = convert_kelvin_to_celsius(minixr.Dataset({"tasmax": (("time", "lat", "lon"), XB)},
                                                           coords={"time": base_time, "lat": lat, "lon": lon}), "tasmax")
        cell_quantiles(base_ds, [0.9], tas="tasmax", period="calendar_day", window=5)            # (warm-up: code objects, allocator)
        sync()
        t0 = time.perf_counter()
        th3 = cell_quantiles(base_ds, [0.9, 0.95, 0.99], tas="tasmax", period="calendar_day", window=5)
        sync()
        res["baseline_build_" + dtype] = {"rows": Y * T, "planes": th3.M, "levels": 3, "entries_per_plane": 5 * Y,
                                          "ms": round(1e3 * (time.perf_counter() - t0), 1), "timed_calls": 1}
        print("baseline_build", dtype, json.dumps(res["baseline_build_" + dtype]), flush=True)
        X = XB[:T].clone()
        del XB, base_ds
        torch.cuda.empty_cache()
        time_values = base_time[:T]
        coords = {"time": time_values, "lat": lat, "lon": lon}
        ds = convert_kelvin_to_celsius(minixr.Dataset({"tasmax": (("time", "lat", "lon"), X)}, coords=coords), "tasmax")
        in_win = torch.from_numpy(in_season(np.ascontiguousarray(sw.windows.reshape(-1)), pkg.day_of_year(time_values))).cuda()
        in_win = in_win.reshape(T, len(lat), len(lon))
        prow = torch.from_numpy(resolve_row_planes(th3.labels, time_values).astype(np.int64)).cuda()
        for wname, season in (("season", sw), ("allyear", None)):
            for sname, L, levels in CASES:
                K = len(levels)
                th = CellThresholds(th3.values[:K], th3.shift, th3.levels[:K], th3.labels, th3.lat, th3.lon, th3.dims)
                one_plane = CellThresholds(th3.values[:K, :1].contiguous(), th3.shift, th3.levels[:K], np.array([0]), th3.lat, th3.lon, th3.dims)
                thr = th.values.reshape(K, th.M, len(lat), len(lon))
                rel = lambda cells: tas_relative_spell_aggregate(ds, th, "popwt", "hierid", df, min_length=L, stat="days", tas="tasmax",
                                                                 period="year", planes="calendar_day", season=season, cells=cells)
                by_period = lambda: tas_relative_spell_aggregate(ds, one_plane, "popwt", "hierid", df, min_length=L, stat="days",
                                                                 tas="tasmax", period="year", season=season)

                def per_threshold():
                    out = []
                    for k in range(K):
                        hot = X >= thr[k].index_select(0, prow)
                        if season is not None:
                            hot &= in_win
                        m = (run_lengths(hot) >= L).to(X.dtype)
                        one = minixr.Dataset({"tas": (("time", "lat", "lon"), m)}, coords=coords)
                        out.append(pkg.weighted_aggregate_grid_to_regions_periods(one, "tas", "popwt", "hierid", df, period="year", season=season))
                    return out

                a = rel("all")["tas-relative-spell"].values
                r_ = rel("referenced")["tas-relative-spell"].values
                b = np.stack([o["tas"].values for o in per_threshold()])
                r = measure({"doy_all": lambda: rel("all"), "doy_referenced": lambda: rel("referenced"),
                             "per_threshold": per_threshold, "by_period": by_period}, sync, N_TIMED)
                fin = np.isfinite(a) & np.isfinite(b)
                r["max_abs_diff_days_doy_all_vs_per_threshold"] = float(np.abs(a - b)[fin].max())
                r["max_abs_diff_days_referenced_vs_all"] = float(np.abs(r_ - a)[np.isfinite(a) & np.isfinite(r_)].max())
                r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
                r["mean_days_per_region_by_level"] = [round(float(v), 3) for v in np.nanmean(a, axis=(1, 2))]
                for k in ("doy_all", "doy_referenced"):
                    r["per_threshold_over_" + k] = round(r["per_threshold"]["median_ms"] / r[k]["median_ms"], 3)
                    r[k + "_leads_per_threshold"] = leads(r[k], r["per_threshold"])
                    r["per_threshold_leads_" + k] = leads(r["per_threshold"], r[k])
                    r[k + "_over_by_period"] = round(r[k]["median_ms"] / r["by_period"]["median_ms"], 3)
                r["by_period_leads_doy_all"] = leads(r["by_period"], r["doy_all"])
                r["referenced_leads_all"] = leads(r["doy_referenced"], r["doy_all"])
                key = "%s_%s_%s" % (dtype, wname, sname)
                res[key] = r
                print(key, json.dumps(r), flush=True)
                dump()
                del th, thr, one_plane
        del ds, X, th3
        pkg.clear_caches()
        torch.cuda.empty_cache()
    dump()
    print("wrote", path)


if __name__ == "__main__":
    main()
