#!/usr/bin/env python3
"""Period quantiles (the annual 5th, 50th, 95th and 99th percentile of a cell's days), at c2-real shape (T = 365, 720 x 1440 cells,
the synthetic impact-region table; fp32 and fp64) of a device-resident Kelvin field shifted by ``convert_kelvin_to_celsius``,
``method="linear"`` -- with the synthetic 150-day season windows of tools/season_timing.py ("season") and without a season
("allyear").  Three arms in one process, alternating inside every round:

  quantile_all          (a) ``tas_quantile_aggregate(..., period="year", cells="all")``: one launch holds every cell's year in
                        LDS and selects the four levels exactly, one apply contracts the 4 rows
  quantile_referenced   (a) the same with ``cells="referenced"``: the field packed to the quads the table references first
  torch                 (b) what a user does without the call.  All year: ``torch.quantile`` along time on the device, in column
                        chunks of at most 16e6 elements (torch.quantile refuses a larger input).  With a season: the field with
                        +inf out of season, ``torch.sort`` along time, the per-cell count of in-season days as the index base,
                        two gathers and a lerp per level, NaN where a cell has no day.  Either way the Kelvin shift and the
                        (4, G) field handed to ONE ``weighted_aggregate_grid_to_regions`` call (4 "time" steps): the yardstick.
                        torch interpolates in the field's type; the largest difference between the arms' results is reported,
                        not asserted.

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; reported as median, min
and max in ms.  No ratio is asked for; the JSON records what was measured, and per case whether a median leads by the project's
rule: by more than the larger min-max spread of the two arms.  Writes the JSON to the path given as the first argument (default
profiles/quantile_timing.json) after every case; ``--only float32`` / ``--only float64`` runs one element type."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_quantile_aggregate  # noqa: E402
from season_timing import growing_days, in_season, measure  # noqa: E402

T, N_TIMED, KELVIN = 365, 12, 273.15
LEVELS = [0.05, 0.5, 0.95, 0.99]
QUANTILE_INPUT_MAX = 16_000_000              # torch.quantile: "input tensor is too large" beyond this many elements


def leads(a, b):
    """does arm ``a``'s median lead arm ``b``'s by more than the larger min-max spread of the two?"""
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    return bool(b["median_ms"] - a["median_ms"] > spread)


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "quantile_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    in_win = torch.from_numpy(in_season(np.ascontiguousarray(sw.windows.reshape(-1)), pkg.day_of_year(time_values))).cuda()      # (T, G)
    days = in_win.sum(0)                                                          # in-season days per cell
    res = {"T": T, "G": G, "periods": 1, "levels": LEVELS, "method": "linear", "timed_calls": N_TIMED, "warm_up_s": 0.3,
           "what": "annual 5th, 50th, 95th and 99th percentile of the days of a device-resident (365 x G) Kelvin field per cell, "
                   "aggregated to regions; ms per call, host clock around a device synchronise; torch = torch.quantile along time in "
                   "column chunks (all year) or a masked torch.sort with per-cell indices (season) + one "
                   "weighted_aggregate_grid_to_regions; leads: the median is ahead by more than the larger min-max spread of the two arms"}
    sync = torch.cuda.synchronize

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        X = engine.synth_field(T, G, seed=11, base=297.0, amp=50.0, dtype=dtype).reshape(T, len(lat), len(lon))
        flat = X.reshape(T, G)
        coords = {"time": time_values, "lat": lat, "lon": lon}
        ds = convert_kelvin_to_celsius(minixr.Dataset({"tas": (("time", "lat", "lon"), X)}, coords=coords), "tas")
        four = {"time": time_values[:len(LEVELS)], "lat": lat, "lon": lon}
        qt = torch.tensor(LEVELS, dtype=X.dtype, device=X.device)
        step = QUANTILE_INPUT_MAX // T
        for wname, season in (("season", sw), ("allyear", None)):
            call = lambda cells: tas_quantile_aggregate(ds, LEVELS, "popwt", "hierid", df, period="year", season=season, cells=cells)

            def with_torch():
                if season is None:
                    v = torch.cat([torch.quantile(flat[:, j:j + step], qt, dim=0) for j in range(0, G, step)], dim=1)      # (4, G)
                else:
                    s = torch.where(in_win, flat, torch.full((), float("inf"), dtype=X.dtype, device=X.device)).sort(dim=0).values
                    h = (days - 1).clamp(min=0).to(X.dtype)[None, :] * qt[:, None]                                         # (4, G)
                    lo = h.floor()
                    g = h - lo
                    lo = lo.long()
                    hi = torch.minimum(lo + 1, (days - 1).clamp(min=0)[None, :])
                    a, b = s.gather(0, lo), s.gather(0, hi)
                    v = torch.where(days[None, :] > 0, a + (b - a) * g, torch.full((), float("nan"), dtype=X.dtype, device=X.device))
                v = (v - KELVIN).reshape(len(LEVELS), len(lat), len(lon))
                one = minixr.Dataset({"tas": (("time", "lat", "lon"), v)}, coords=four)
                return pkg.weighted_aggregate_grid_to_regions(one, "tas", "popwt", "hierid", df)

            a = call("all")["tas-quantile"].values
            r_ = call("referenced")["tas-quantile"].values
            yard = with_torch()["tas"]
            b = np.asarray(yard.values)
            b = (b if tuple(yard.dims)[0] == "time" else b.T).reshape(a.shape)        # (4, R) -> the call's (4, 1 | R, R | 1)
            r = measure({"quantile_all": lambda: call("all"), "quantile_referenced": lambda: call("referenced"), "torch": with_torch},
                        sync, N_TIMED)
            fin = np.isfinite(a) & np.isfinite(b)
            r["max_abs_diff_degC_quantile_all_vs_torch"] = float(np.abs(a - b)[fin].max())
            r["max_abs_diff_degC_referenced_vs_all"] = float(np.abs(r_ - a)[np.isfinite(a) & np.isfinite(r_)].max())
            r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
            r["mean_degC_per_region_by_level"] = [round(float(v), 3) for v in np.nanmean(a, axis=(1, 2))]
            for k in ("quantile_all", "quantile_referenced"):
                r["torch_over_" + k] = round(r["torch"]["median_ms"] / r[k]["median_ms"], 3)
                r[k + "_leads_torch"] = leads(r[k], r["torch"])
                r["torch_leads_" + k] = leads(r["torch"], r[k])
            r["quantile_referenced_leads_quantile_all"] = leads(r["quantile_referenced"], r["quantile_all"])
            key = "%s_%s" % (dtype, wname)
            res[key] = r
            print(key, json.dumps(r), flush=True)
            dump()
        del ds, X, flat
        pkg.clear_caches()
        torch.cuda.empty_cache()
    dump()
    print("wrote", path)


if __name__ == "__main__":
    main()
