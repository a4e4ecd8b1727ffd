#!/usr/bin/env python3
"""Rolling-window extremes (the hottest N-day mean), annual at c2-real shape (T = 365, 720 x 1440 cells, the synthetic
impact-region table; fp32 and fp64) of a device-resident tasmax-like Kelvin field shifted by ``convert_kelvin_to_celsius``:
windows 1, 3, 5, 7 days, ``stat="max"``, ``of="mean"`` -- with the synthetic 150-day season windows of tools/season_timing.py
("season") and without a season ("allyear").  Three arms in one process, alternating inside every round:

  rolling_all          (a) ``tas_rolling_aggregate(..., period="year", cells="all")``: one launch walks the year once with a ring
                       of 8 days and an extreme per chain length in registers, one apply contracts the 4 rows
  rolling_referenced   (a) the same with ``cells="referenced"``: the field packed to the quads the table references first
  per_window           (b) what a user does without the call: per window a (T - W + 1, G) rolling mean on the device with torch
                       (``unfold`` + ``mean``; with a season the windows that hold an out-of-season day are set to -inf by an
                       unfolded mask), an ``amax`` over the year, the Kelvin shift, NaN where no window exists, and the (1, G)
                       field handed to ``weighted_aggregate_grid_to_regions``: 4 rolling means and 4 aggregation calls, the
                       yardstick.  torch forms the mean in the field's type; the largest difference between the arms' results
                       is reported, not asserted.

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; reported as median, min
and max in ms.  No ratio is asked for; the JSON records what was measured, and per case whether a median leads by the project's
rule: by more than the larger min-max spread of the two arms.  Writes the JSON to the path given as the first argument (default
profiles/rolling_timing.json) after every case; ``--only float32`` / ``--only float64`` runs one element type."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_rolling_aggregate  # noqa: E402
from season_timing import growing_days, in_season, measure  # noqa: E402

T, N_TIMED, KELVIN = 365, 12, 273.15
WINDOWS = [1, 3, 5, 7]


def leads(a, b):
    """does arm ``a``'s median lead arm ``b``'s by more than the larger min-max spread of the two?"""
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    return bool(b["median_ms"] - a["median_ms"] > spread)


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "rolling_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    in_win = torch.from_numpy(in_season(np.ascontiguousarray(sw.windows.reshape(-1)), pkg.day_of_year(time_values))).cuda()
    in_win = in_win.reshape(T, len(lat), len(lon))
    res = {"T": T, "G": G, "periods": 1, "windows": WINDOWS, "stat": "max", "of": "mean", "timed_calls": N_TIMED, "warm_up_s": 0.3,
           "what": "annual maximum of the 1-, 3-, 5- and 7-day running mean of a device-resident (365 x G) Kelvin field, aggregated to "
                   "regions; ms per call, host clock around a device synchronise; per_window = 4 torch rolling means (unfold + mean) "
                   "+ amax + 4 weighted_aggregate_grid_to_regions; leads: the median is ahead by more than the larger min-max spread "
                   "of the two arms"}
    sync = torch.cuda.synchronize

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        X = engine.synth_field(T, G, seed=11, base=297.0, amp=50.0, dtype=dtype).reshape(T, len(lat), len(lon))
        coords = {"time": time_values, "lat": lat, "lon": lon}
        ds = convert_kelvin_to_celsius(minixr.Dataset({"tasmax": (("time", "lat", "lon"), X)}, coords=coords), "tasmax")
        one_day = {"time": time_values[:1], "lat": lat, "lon": lon}
        for wname, season in (("season", sw), ("allyear", None)):
            rolling = lambda cells: tas_rolling_aggregate(ds, WINDOWS, "popwt", "hierid", df, stat="max", of="mean", tas="tasmax",
                                                          period="year", season=season, cells=cells)

            def per_window():
                out = []
                for W in WINDOWS:
                    mean = X.unfold(0, W, 1).mean(-1)                             # (T - W + 1, lat, lon)
                    if season is not None:
                        whole = in_win.unfold(0, W, 1).all(-1)
                        mean = torch.where(whole, mean, torch.full((), float("-inf"), dtype=X.dtype, device=X.device))
                    m = mean.amax(0)
                    m = torch.where(torch.isinf(m), torch.full((), float("nan"), dtype=X.dtype, device=X.device), m - KELVIN)
                    one = minixr.Dataset({"tas": (("time", "lat", "lon"), m[None])}, coords=one_day)
                    out.append(pkg.weighted_aggregate_grid_to_regions(one, "tas", "popwt", "hierid", df))
                return out

            a = rolling("all")["tas-rolling"].values
            r_ = rolling("referenced")["tas-rolling"].values
            b = np.stack([np.asarray(o["tas"].values).reshape(a.shape[1:]) for o in per_window()])
            r = measure({"rolling_all": lambda: rolling("all"), "rolling_referenced": lambda: rolling("referenced"),
                         "per_window": per_window}, sync, N_TIMED)
            fin = np.isfinite(a) & np.isfinite(b)
            r["max_abs_diff_degC_rolling_all_vs_per_window"] = float(np.abs(a - b)[fin].max())
            r["max_abs_diff_degC_referenced_vs_all"] = float(np.abs(r_ - a)[np.isfinite(a) & np.isfinite(r_)].max())
            r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
            r["mean_degC_per_region_by_window"] = [round(float(v), 3) for v in np.nanmean(a, axis=(1, 2))]
            for k in ("rolling_all", "rolling_referenced"):
                r["per_window_over_" + k] = round(r["per_window"]["median_ms"] / r[k]["median_ms"], 3)
                r[k + "_leads_per_window"] = leads(r[k], r["per_window"])
            r["rolling_referenced_leads_rolling_all"] = leads(r["rolling_referenced"], r["rolling_all"])
            key = "%s_%s" % (dtype, wname)
            res[key] = r
            print(key, json.dumps(r), flush=True)
            dump()
        del ds, X
        pkg.clear_caches()
        torch.cuda.empty_cache()
    dump()
    print("wrote", path)


if __name__ == "__main__":
    main()
