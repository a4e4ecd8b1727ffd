#!/usr/bin/env python3
"""Sinusoid exposure bins, annual totals at c2-real shape (T = 365, 720 x 1440 cells, the synthetic impact-region table; fp32 and
fp64) of device-resident Kelvin ``tasmin`` / ``tasmax`` shifted by ``convert_kelvin_to_celsius``: 42 bins -- 40 of 1 C over
0 .. 40 C and the two open ends -- with the synthetic 150-day season windows of tools/season_timing.py ("season") and without a
season ("allyear").  Four arms in one process, alternating inside every round:

  exposure_all          ``snyder_exposure_aggregate(..., period="year", cells="all")``: one launch sums all 42 bins, one apply
                        contracts the 42 rows
  exposure_referenced   the same with ``cells="referenced"``: both fields packed to the quads the table references first
  per_edge              what a user does without the call, the yardstick: per edge the torch expression of A on the device
                        (``where(isnan, 0, where(~(lo < e), 1, where(~(hi > e), 0, acos(clamp((e - M) / w, -1, 1)) / pi)))``
                        on the shifted fields) handed to ``weighted_aggregate_grid_to_regions_periods(..., period="year")``,
                        then differenced: 43 fields and 43 period calls
  edd_ladder            context, not a yardstick: ``snyder_edd_aggregate`` at the 41 finite edges on the same fields -- the
                        same loads, similar arithmetic

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; reported as median, min
and max in ms.  THE VERDICT per case and exposure arm, by the project's rule: "ahead" only if its median leads the yardstick's
by more than the larger min-max spread of the two, else "not ahead".  No speed-up is asked for; the JSON records what was
measured.  Writes the JSON to the path given as the first argument (default profiles/exposure_timing.json) after every case;
``--only float32`` / ``--only float64`` runs one element type."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, snyder_edd_aggregate, snyder_exposure_aggregate  # noqa: E402
from season_timing import growing_days, measure  # noqa: E402

T, N_TIMED, KELVIN = 365, 12, 273.15
EDGES = [-float("inf")] + [float(e) for e in range(0, 41)] + [float("inf")]


def verdict(arm, yardstick):
    spread = max(arm["max_ms"] - arm["min_ms"], yardstick["max_ms"] - yardstick["min_ms"])
    return "ahead" if yardstick["median_ms"] - arm["median_ms"] > spread else "not ahead"


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "exposure_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    res = {"T": T, "G": G, "periods": 1, "bins": len(EDGES) - 1, "edges": [repr(e) for e in EDGES], "timed_calls": N_TIMED, "warm_up_s": 0.3,
           "what": "annual exposure (days) in 42 temperature bins of device-resident (365 x G) Kelvin tasmin / tasmax, aggregated to "
                   "regions; ms per call, host clock around a device synchronise; per_edge = 43 torch fields + 43 "
                   "weighted_aggregate_grid_to_regions_periods, differenced; edd_ladder = snyder_edd_aggregate at the 41 finite edges",
           "rule": "ahead only if the median leads by more than the larger min-max spread of the two arms"}
    sync = torch.cuda.synchronize

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        shape = (T, len(lat), len(lon))
        lo = engine.synth_field(T, G, seed=11, base=281.0, amp=40.0, dtype=dtype).reshape(shape)
        hi = lo + engine.synth_field(T, G, seed=12, base=8.0, amp=14.0, dtype=dtype).reshape(shape).abs()
        coords = {"time": time_values, "lat": lat, "lon": lon}
        ds = minixr.Dataset({"tasmin": (("time", "lat", "lon"), lo), "tasmax": (("time", "lat", "lon"), hi)}, coords=coords)
        for k in ("tasmin", "tasmax"):
            ds[k].attrs["units"] = "K"
            ds = convert_kelvin_to_celsius(ds, k)
        for wname, season in (("season", sw), ("allyear", None)):
            expo = lambda cells: snyder_exposure_aggregate(ds, EDGES, "popwt", "hierid", df, period="year", season=season, cells=cells)
            ladder = lambda: snyder_edd_aggregate(ds, EDGES[1:-1], "popwt", "hierid", df, period="year", season=season)

            def per_edge():
                clo, chi = lo - KELVIN, hi - KELVIN
                M, w = (chi + clo) / 2, (chi - clo) / 2
                A = []
                for e in EDGES:
                    band = torch.acos(torch.clamp((e - M) / w, -1.0, 1.0)) / math.pi
                    a = torch.where(~(clo < e), torch.ones_like(clo), torch.where(~(chi > e), torch.zeros_like(clo), band))
                    a = torch.where(torch.isnan(clo) | torch.isnan(chi), torch.zeros_like(clo), a)
                    one = minixr.Dataset({"a": (("time", "lat", "lon"), a)}, coords=coords)
                    A.append(pkg.weighted_aggregate_grid_to_regions_periods(one, "a", "popwt", "hierid", df, period="year", season=season)["a"].values)
                return np.stack([A[k] - A[k + 1] for k in range(len(A) - 1)])

            a = expo("all")["exposure"].values
            r_ = expo("referenced")["exposure"].values
            b = per_edge()
            r = measure({"exposure_all": lambda: expo("all"), "exposure_referenced": lambda: expo("referenced"), "per_edge": per_edge,
                         "edd_ladder": ladder}, sync, N_TIMED)
            fin = np.isfinite(a) & np.isfinite(b)
            r["max_abs_diff_days_exposure_all_vs_per_edge"] = float(np.abs(a - b)[fin].max())
            r["max_abs_diff_days_referenced_vs_all"] = float(np.abs(r_ - a)[np.isfinite(a) & np.isfinite(r_)].max())
            r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
            r["mean_days_per_region_all_bins"] = float(np.nansum(a, axis=0).mean())
            for k in ("exposure_all", "exposure_referenced"):
                r["per_edge_over_" + k] = round(r["per_edge"]["median_ms"] / r[k]["median_ms"], 3)
                r["verdict_" + k] = verdict(r[k], r["per_edge"])
            key = "%s_%s" % (dtype, wname)
            res[key] = r
            print(key, json.dumps(r), flush=True)
            dump()
        del ds, lo, hi
        pkg.clear_caches()
        torch.cuda.empty_cache()
    dump()
    print("wrote", path)


if __name__ == "__main__":
    main()
