#!/usr/bin/env python3
"""Spell days (heat-wave days), annual totals at c2-real shape (T = 365, 720 x 1440 cells, the synthetic impact-region table; fp32
and fp64) of a device-resident tasmax-like Kelvin field shifted by ``convert_kelvin_to_celsius``: 11 thresholds, 30 .. 40 C,
``min_length=3``, ``stat="days"`` -- with the synthetic 150-day season windows of tools/season_timing.py ("season") and without a
season ("allyear").  Three arms in one process, alternating inside every round:

  spell_all          (a) ``tas_spell_aggregate(..., period="year", cells="all")``: one launch walks the year once per group of 8
                     thresholds with a run counter per cell and threshold, one apply contracts the 11 rows
  spell_referenced   (a) the same with ``cells="referenced"``: the field packed to the quads the table references first
  per_threshold      (b) what a user does without the call: per threshold a run-length scan on the device with torch -- hot =
                     ``x >= thr`` (and in season), the length of the run a day belongs to from a forward and a backward
                     ``cumsum`` / ``cummax`` pass in int16, the 0/1 field ``hot & (length >= 3)`` -- handed to
                     ``weighted_aggregate_grid_to_regions_periods(..., period="year")``: 11 scans and 11 period calls, the
                     yardstick.  torch compares in the field's type, so in fp32 a value next to a threshold may fall on the
                     other side than in arm (a) and split or join a run; the largest difference between the arms' results is
                     reported, not asserted -- once as the user would write it, once (untimed) with the threshold rounded up to
                     the element type as arm (a) compares (``engine.bin_thresholds``).

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; reported as median, min
and max in ms.  No ratio is asked for; the JSON records what was measured, and per case whether a median leads by the project's
rule: by more than the larger min-max spread of the two arms.  Writes the JSON to the path given as the first argument (default
profiles/spell_timing.json) after every case; ``--only float32`` / ``--only float64`` runs one element type."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_spell_aggregate  # noqa: E402
from season_timing import growing_days, in_season, measure  # noqa: E402

T, N_TIMED, KELVIN, MIN_LENGTH = 365, 12, 273.15, 3
THRESHOLDS = [float(t) for t in range(30, 41)]


def run_lengths(hot):
    """(T, ...) bool -> int16 of the same shape: the length of the run of consecutive True along axis 0 a position belongs to
    (0 where False); T < 32768"""
    import torch

    def upto(h):                                                                  # the run's length up to and including each position
        c = h.cumsum(0, dtype=torch.int16)
        return c - torch.where(h, torch.zeros_like(c), c).cummax(0).values
    back = torch.flip(upto(torch.flip(hot, (0,))), (0,))
    return torch.where(hot, upto(hot) + back - 1, torch.zeros((), dtype=torch.int16, device=hot.device))


def leads(a, b):
    """does arm ``a``'s median lead arm ``b``'s by more than the larger min-max spread of the two?"""
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    return bool(b["median_ms"] - a["median_ms"] > spread)


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "spell_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    in_win = torch.from_numpy(in_season(np.ascontiguousarray(sw.windows.reshape(-1)), pkg.day_of_year(time_values))).cuda()
    in_win = in_win.reshape(T, len(lat), len(lon))
    res = {"T": T, "G": G, "periods": 1, "thresholds": THRESHOLDS, "min_length": MIN_LENGTH, "stat": "days", "timed_calls": N_TIMED,
           "warm_up_s": 0.3,
           "what": "annual heat-wave days (runs of >= 3 days at or above each of 11 thresholds) of a device-resident (365 x G) Kelvin "
                   "field, aggregated to regions; ms per call, host clock around a device synchronise; per_threshold = 11 torch "
                   "run-length scans + 11 weighted_aggregate_grid_to_regions_periods; leads: the median is ahead by more than the "
                   "larger min-max spread of the two arms"}
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
        for wname, season in (("season", sw), ("allyear", None)):
            spell = lambda cells: tas_spell_aggregate(ds, THRESHOLDS, "popwt", "hierid", df, min_length=MIN_LENGTH, stat="days",
                                                      tas="tasmax", period="year", season=season, cells=cells)

            def per_threshold(exact=False):
                out = []
                for thr in THRESHOLDS:
                    hot = X >= (float(engine.bin_thresholds([thr], -KELVIN, dtype)[0]) if exact else thr + KELVIN)
                    if season is not None:
                        hot &= in_win
                    m = (run_lengths(hot) >= MIN_LENGTH).to(X.dtype)
                    one = minixr.Dataset({"tas": (("time", "lat", "lon"), m)}, coords=coords)
                    out.append(pkg.weighted_aggregate_grid_to_regions_periods(one, "tas", "popwt", "hierid", df, period="year", season=season))
                return out

            a = spell("all")["tas-spell"].values
            r_ = spell("referenced")["tas-spell"].values
            b = np.stack([o["tas"].values for o in per_threshold()])
            r = measure({"spell_all": lambda: spell("all"), "spell_referenced": lambda: spell("referenced"), "per_threshold": per_threshold},
                        sync, N_TIMED)
            fin = np.isfinite(a) & np.isfinite(b)
            r["max_abs_diff_days_spell_all_vs_per_threshold"] = float(np.abs(a - b)[fin].max())
            b_exact = np.stack([o["tas"].values for o in per_threshold(exact=True)])       # (not timed: the yardstick on arm (a)'s comparison)
            r["max_abs_diff_days_spell_all_vs_per_threshold_exact_compare"] = float(np.abs(a - b_exact)[np.isfinite(a) & np.isfinite(b_exact)].max())
            r["max_abs_diff_days_referenced_vs_all"] = float(np.abs(r_ - a)[np.isfinite(a) & np.isfinite(r_)].max())
            r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
            r["mean_days_per_region_by_threshold"] = [round(float(v), 3) for v in np.nanmean(a, axis=(1, 2))]
            for k in ("spell_all", "spell_referenced"):
                r["per_threshold_over_" + k] = round(r["per_threshold"]["median_ms"] / r[k]["median_ms"], 3)
                r[k + "_leads_per_threshold"] = leads(r[k], r["per_threshold"])
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
