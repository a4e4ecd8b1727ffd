#!/usr/bin/env python3
"""Spell days against PER-CELL thresholds, annual totals at c2-real shape (T = 365, 720 x 1440 cells, the synthetic impact-region
table; fp32 and fp64) of a device-resident tasmax-like Kelvin field shifted by ``convert_kelvin_to_celsius``.  The thresholds are
each cell's own 90th / 95th / 99th percentile of the same year (``relative.cell_quantiles``, untimed).  Two statistics: WSDI-like
days (``min_length=6``) and TX90p-like days (``min_length=1``) -- with the synthetic 150-day season windows of
tools/season_timing.py ("season") and without a season ("allyear").  Four arms in one process, alternating inside every round:

  relative_all         ``tas_relative_spell_aggregate(..., period="year", cells="all")``: one launch, the thresholds read per cell
  relative_referenced  the same with ``cells="referenced"``
  per_threshold        what a user does today: per level ``hot = x >= thr[k][None]`` on the device (and in season), the run-length
                       scan of tools/spell_timing.py, the 0/1 field handed to ``weighted_aggregate_grid_to_regions_periods``: the
                       yardstick.  Field and thresholds are raw elements of one variable, so both arms classify alike.
  scalar_spell         for context, not a rival: ``tas_spell_aggregate`` at three scalar thresholds -- the same loads, the
                       thresholds in scalar registers

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; median, min and max in ms.
A third case, "tx90p8", takes EIGHT levels (0.5 .. 0.99) with ``min_length=1``: three levels fit one group of the kernel whatever
its size, eight are two groups of 4 or one of 8, so only this case can tell the group sizes apart.
Nothing is promised: the JSON records what was measured, and per case whether a median leads by the project's rule -- by more than
the larger min-max spread of the two arms.  ``group`` in the JSON is the library's WAGG_CELL_SPELL_GROUP.  To compare group sizes,
build a second library with the other value of that constant and run this tool on it: ``--lib PATH --group N`` loads that
library instead of the package's and records N (the tool cannot read the constant out of a library); ``--compare A.json B.json``
prints, per case and arm, which of two such records leads by the rule.  Writes the JSON to the path given as the first argument
(default profiles/relative_timing.json) after every case; ``--only float32`` / ``--only float64`` runs one type.  The synthetic field
has no day-to-day persistence, so runs of six days above a cell's 90th percentile hardly occur: the "wsdi6" cases time the kernel
(which does the same work whatever it counts) but their agreement figures compare zeros; the "tx90p" cases carry the agreement."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import _lib, engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.relative import cell_quantiles  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_relative_spell_aggregate, tas_spell_aggregate  # noqa: E402
from season_timing import growing_days, in_season, measure  # noqa: E402
from spell_timing import leads, run_lengths  # noqa: E402

T, N_TIMED = 365, 12
LEVELS = [0.9, 0.95, 0.99]
LEVELS8 = [0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99]
SCALAR = [30.0, 35.0, 40.0]
SCALAR8 = [26.0, 28.0, 30.0, 32.0, 34.0, 36.0, 38.0, 40.0]
ARMS = ("relative_all", "relative_referenced", "per_threshold", "scalar_spell")


def compare(path_a, path_b):
    """per case and arm: does record A's median lead record B's by the rule, or B's A's?"""
    a, b = json.load(open(path_a)), json.load(open(path_b))
    out = {"a": {"path": os.path.basename(path_a), "group": a.get("group")}, "b": {"path": os.path.basename(path_b), "group": b.get("group")}}
    for key in a:
        if isinstance(a[key], dict) and key in b:
            out[key] = {arm: {"a_median_ms": a[key][arm]["median_ms"], "b_median_ms": b[key][arm]["median_ms"],
                              "a_leads": leads(a[key][arm], b[key][arm]), "b_leads": leads(b[key][arm], a[key][arm])}
                        for arm in ARMS[:2]}
    return out


def main():
    import torch
    args = sys.argv[1:]
    if "--compare" in args:
        i = args.index("--compare")
        print(json.dumps(compare(args[i + 1], args[i + 2]), indent=1))
        return
    only = args[args.index("--only") + 1] if "--only" in args else None
    group = _lib.CELL_SPELL_GROUP
    if "--lib" in args:
        _lib.LIB_PATH = os.path.abspath(args[args.index("--lib") + 1])          # (before the first load)
        group = int(args[args.index("--group") + 1])
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in ("--only", "--lib", "--group"))]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "relative_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    in_win = torch.from_numpy(in_season(np.ascontiguousarray(sw.windows.reshape(-1)), pkg.day_of_year(time_values))).cuda()
    in_win = in_win.reshape(T, len(lat), len(lon))
    res = {"T": T, "G": G, "periods": 1, "levels": LEVELS, "levels8": LEVELS8, "scalar_thresholds": SCALAR, "scalar_thresholds8": SCALAR8, "group": group,
           "library": "the package's" if "--lib" not in args else "another build, WAGG_CELL_SPELL_GROUP = %d" % group, "timed_calls": N_TIMED,
           "warm_up_s": 0.3,
           "what": "annual days in runs of >= L days at or above each cell's own 90th / 95th / 99th percentile of the year, of a "
                   "device-resident (365 x G) Kelvin field, aggregated to regions; ms per call, host clock around a device synchronise; "
                   "per_threshold = per level (x >= thr[None], torch run-length scan, weighted_aggregate_grid_to_regions_periods); leads: the "
                   "median is ahead by more than the larger min-max spread of the two arms"}
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
            for sname, L, levels, scalars in (("wsdi6", 6, LEVELS, SCALAR), ("tx90p", 1, LEVELS, SCALAR), ("tx90p8", 1, LEVELS8, SCALAR8)):
                th = cell_quantiles(ds, levels, tas="tasmax", period=None, method="higher", season=season)
                thr = th.values.reshape(len(levels), len(lat), len(lon))
                rel = lambda cells: tas_relative_spell_aggregate(ds, th, "popwt", "hierid", df, min_length=L, stat="days", tas="tasmax",
                                                                 period="year", season=season, cells=cells)
                scalar = lambda: tas_spell_aggregate(ds, scalars, "popwt", "hierid", df, min_length=L, stat="days", tas="tasmax",
                                                     period="year", season=season)

                def per_threshold():
                    out = []
                    for k in range(len(levels)):
                        hot = X >= thr[k][None]
                        if season is not None:
                            hot &= in_win
                        m = (run_lengths(hot) >= L).to(X.dtype)
                        one = minixr.Dataset({"tas": (("time", "lat", "lon"), m)}, coords=coords)
                        out.append(pkg.weighted_aggregate_grid_to_regions_periods(one, "tas", "popwt", "hierid", df, period="year", season=season))
                    return out

                a = rel("all")["tas-relative-spell"].values
                r_ = rel("referenced")["tas-relative-spell"].values
                b = np.stack([o["tas"].values for o in per_threshold()])
                r = measure({"relative_all": lambda: rel("all"), "relative_referenced": lambda: rel("referenced"),
                             "per_threshold": per_threshold, "scalar_spell": scalar}, sync, N_TIMED)
                fin = np.isfinite(a) & np.isfinite(b)
                r["max_abs_diff_days_relative_all_vs_per_threshold"] = float(np.abs(a - b)[fin].max())
                r["max_abs_diff_days_referenced_vs_all"] = float(np.abs(r_ - a)[np.isfinite(a) & np.isfinite(r_)].max())
                r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
                r["mean_days_per_region_by_level"] = [round(float(v), 3) for v in np.nanmean(a, axis=(1, 2))]
                for k in ("relative_all", "relative_referenced"):
                    r["per_threshold_over_" + k] = round(r["per_threshold"]["median_ms"] / r[k]["median_ms"], 3)
                    r[k + "_leads_per_threshold"] = leads(r[k], r["per_threshold"])
                    r["per_threshold_leads_" + k] = leads(r["per_threshold"], r[k])
                r["referenced_leads_all"] = leads(r["relative_referenced"], r["relative_all"])
                key = "%s_%s_%s" % (dtype, wname, sname)
                res[key] = r
                print(key, json.dumps(r), flush=True)
                dump()
                del th, thr
        del ds, X
        pkg.clear_caches()
        torch.cuda.empty_cache()
    dump()
    print("wrote", path)


if __name__ == "__main__":
    main()
