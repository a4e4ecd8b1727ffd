#!/usr/bin/env python3
"""Temperature-bin day counts, annual totals at c2-real shape (T = 365, 720 x 1440 cells, the synthetic impact-region table; fp32
and fp64) of a device-resident Kelvin field shifted by ``convert_kelvin_to_celsius``: 42 bins -- 40 of 1 C over 0 .. 40 C and the
two open ends -- with the synthetic 150-day season windows of tools/season_timing.py ("season") and without a season
("allyear").  Three arms in one process, alternating inside every round:

  bins_all          (a) ``tas_bins_aggregate(..., period="year", cells="all")``: one launch counts all 42 bins, one apply
                    contracts the 42 rows
  bins_referenced   (a) the same with ``cells="referenced"``: the field packed to the quads the table references first
  per_bin           (b) what a user does without the call: per bin a 0/1 field made on the device with torch
                    (``((x >= lo) & (x < hi)).to(x.dtype)`` on the Kelvin field, the edges shifted to kelvin) handed to
                    ``weighted_aggregate_grid_to_regions_periods(..., period="year")`` -- 42 masks and 42 period calls: the
                    yardstick.  torch compares in the field's type, so in fp32 a value next to an edge may fall on the other
                    side than in arm (a); the largest difference between the arms' results is reported, not asserted.

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; reported as median, min
and max in ms.  No ratio is asked for; the JSON records what was measured.  Writes the JSON to the path given as the first
argument (default profiles/bins_timing.json) after every case; ``--only float32`` / ``--only float64`` runs one element type."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_bins_aggregate  # noqa: E402
from season_timing import growing_days, measure  # noqa: E402

T, N_TIMED, KELVIN = 365, 12, 273.15
EDGES = [-float("inf")] + [float(e) for e in range(0, 41)] + [float("inf")]


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "bins_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    res = {"T": T, "G": G, "periods": 1, "bins": len(EDGES) - 1, "edges": [repr(e) for e in EDGES], "timed_calls": N_TIMED, "warm_up_s": 0.3,
           "what": "annual day counts in 42 temperature bins of a device-resident (365 x G) Kelvin field, aggregated to regions; ms per "
                   "call, host clock around a device synchronise; per_bin = 42 torch masks + 42 weighted_aggregate_grid_to_regions_periods"}
    sync = torch.cuda.synchronize

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        X = engine.synth_field(T, G, seed=11, base=287.0, amp=50.0, dtype=dtype).reshape(T, len(lat), len(lon))
        coords = {"time": time_values, "lat": lat, "lon": lon}
        ds = convert_kelvin_to_celsius(minixr.Dataset({"tas": (("time", "lat", "lon"), X)}, coords=coords), "tas")
        for wname, season in (("season", sw), ("allyear", None)):
            bins = lambda cells: tas_bins_aggregate(ds, EDGES, "popwt", "hierid", df, period="year", season=season, cells=cells)

            def per_bin():
                out = []
                for lo, hi in zip(EDGES[:-1], EDGES[1:]):
                    m = ((X >= lo + KELVIN) & (X < hi + KELVIN)).to(X.dtype)
                    one = minixr.Dataset({"tas": (("time", "lat", "lon"), m)}, coords=coords)
                    out.append(pkg.weighted_aggregate_grid_to_regions_periods(one, "tas", "popwt", "hierid", df, period="year", season=season))
                return out

            a = bins("all")["tas-bins"].values
            r_ = bins("referenced")["tas-bins"].values
            b = np.stack([o["tas"].values for o in per_bin()])
            r = measure({"bins_all": lambda: bins("all"), "bins_referenced": lambda: bins("referenced"), "per_bin": per_bin}, sync, N_TIMED)
            fin = np.isfinite(a) & np.isfinite(b)
            r["max_abs_diff_days_bins_all_vs_per_bin"] = float(np.abs(a - b)[fin].max())
            r["max_abs_diff_days_referenced_vs_all"] = float(np.abs(r_ - a)[np.isfinite(a) & np.isfinite(r_)].max())
            r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
            r["mean_days_per_region_all_bins"] = float(np.nansum(a, axis=0).mean())
            for k in ("bins_all", "bins_referenced"):
                r["per_bin_over_" + k] = round(r["per_bin"]["median_ms"] / r[k]["median_ms"], 3)
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
