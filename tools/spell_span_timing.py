#!/usr/bin/env python3
"""Spells that run across period boundaries, annual values at c2-real shape (720 x 1440 cells, the synthetic impact-region table)
of a device-resident pr-like field of several years, ``period="year"``: what ``tas_spell_aggregate(..., span="record")`` costs
beside the truncating call and beside what a user writes today.  The field has day-to-day persistence -- an AR(1) series per
cell (lag-one correlation 0.8), cut at zero and scaled to mm/day, about 60 % of the days dry (pr < 1 mm) -- so that runs do
cross the year ends; the share of cells with a run across at least one year end is recorded per case.  An iid field has almost
no such run, and its agreement would compare the trivial case.  fp32: 10 years (T = 3650); fp64: ``--years64`` years (default
5: half the bytes of the record, the yardstick's intermediates are what asks for it).

Cases: CDD (``stat="longest"``, ``side="below"``, threshold 1 mm), CWD (the same, ``side="above"``), and wet-spell days in the
form of heat-wave days (``stat="days"``, ``min_length=6``, 11 thresholds 0.5 .. 5.5 mm, ``side="above"``).  Four arms in one
process, alternating inside every round:

  record_all          ``span="record", cells="all"``: one launch of column block x threshold group blocks, each walking the record
  record_referenced   ``span="record", cells="referenced"``: the same on the packed row -- few blocks, the known weakness
  period_all          ``span="period", cells="all"``: the truncating call, whose grid has the period dimension
  per_threshold       the yardstick, what a user writes today: per threshold tools/spell_timing.py's torch run-length scan over
                      the WHOLE record without a reset at year ends -- the running length for "longest", reduced per year by a
                      max; the 0 / 1 field ``hot & (whole length >= 6)`` for "days", summed per year -- and one
                      ``weighted_aggregate_grid_to_regions_periods`` call per threshold on the result

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; median, min and max in ms.
No ratio is asked for; the JSON records what was measured, the agreement of results and NaN patterns with the yardstick, and per
pair of arms whether a median leads by the project's rule: by more than the larger min-max spread of the two.  Writes the JSON
to the path given as the first argument (default profiles/spell_span_timing.json) after every case; ``--only float32`` /
``--only float64`` runs one element type."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import minixr, synth  # noqa: E402
from climate_toolbox_amd.transformations import tas_spell_aggregate  # noqa: E402
from season_timing import measure  # noqa: E402
from spell_timing import leads  # noqa: E402

N_TIMED, DAYS_PER_YEAR = 12, 365
CASES = (("cdd", dict(stat="longest", side="below"), [1.0], 1), ("cwd", dict(stat="longest", side="above"), [1.0], 1),
         ("wet_spell_days", dict(stat="days", side="above", min_length=6), [0.5 + 0.5 * k for k in range(11)], 6))


def pr_like(torch, T, G, dtype, seed):
    """(T, G) device tensor: AR(1) per cell, x[t] = 0.8 x[t - 1] + 0.6 e[t] (unit variance), pr = max(x + 0.25, 0) * 4 mm/day,
    filled row by row"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    X = torch.empty((T, G), dtype=dtype, device="cuda")
    x = torch.randn(G, dtype=torch.float32, device="cuda", generator=g)
    for t in range(T):
        x = 0.8 * x + 0.6 * torch.randn(G, dtype=torch.float32, device="cuda", generator=g)
        X[t] = torch.clamp(x + 0.25, min=0.0) * 4.0
    return X


def upto(h):
    """(T, ...) bool -> int16: the running length of the run of True along axis 0 at each position (0 where False); T < 32768"""
    import torch
    c = h.cumsum(0, dtype=torch.int16)
    return c - torch.where(h, torch.zeros_like(c), c).cummax(0).values


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    years64 = int(args[args.index("--years64") + 1]) if "--years64" in args else 5
    flagged = {i + 1 for i, a in enumerate(args) if a in ("--only", "--years64")}
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and i not in flagged]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "spell_span_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    res = {"G": G, "timed_calls": N_TIMED, "warm_up_s": 0.3, "years": {"float32": 10, "float64": years64},
           "what": "annual spell statistics of a device-resident (365 * years x G) pr-like AR(1) field, period='year', aggregated to "
                   "regions; ms per call, host clock around a device synchronise; per_threshold = per threshold a torch run-length "
                   "scan over the whole record, the per-year reduction and one weighted_aggregate_grid_to_regions_periods call; "
                   "leads: the median is ahead by more than the larger min-max spread of the two arms"}
    sync = torch.cuda.synchronize

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        years = res["years"][dtype]
        T = DAYS_PER_YEAR * years
        days = np.datetime64("2001-01-01") + np.arange(T + years)
        month = days.astype("datetime64[M]")
        feb29 = (month.astype(int) % 12 == 1) & ((days - month).astype(int) == 28)
        time_values = days[~feb29][:T]                                            # a 365-day calendar: every year has 365 rows
        tdt = torch.float32 if dtype == "float32" else torch.float64
        X = pr_like(torch, T, G, tdt, seed=11).reshape(T, len(lat), len(lon))
        coords = {"time": time_values, "lat": lat, "lon": lon}
        ds = minixr.Dataset({"pr": (("time", "lat", "lon"), X)}, coords=coords)
        year_time = np.array([np.datetime64("%d-07-01" % (2001 + y)) for y in range(years)])
        ycoords = {"time": year_time, "lat": lat, "lon": lon}
        for cname, kw, thresholds, L in CASES:
            call = lambda span, cells: tas_spell_aggregate(ds, thresholds, "popwt", "hierid", df, tas="pr", period="year", span=span,
                                                           cells=cells, **kw)

            def hot_of(thr):
                return X < thr if kw["side"] == "below" else X >= thr

            def per_threshold():
                out = []
                for thr in thresholds:
                    hot = hot_of(thr)
                    run = upto(hot)
                    if kw["stat"] == "longest":
                        f = run.reshape(years, DAYS_PER_YEAR, len(lat), len(lon)).amax(1).to(X.dtype)
                    else:
                        back = torch.flip(upto(torch.flip(hot, (0,))), (0,))
                        m = (hot & (run + back - 1 >= L)).to(X.dtype)
                        f = m.reshape(years, DAYS_PER_YEAR, len(lat), len(lon)).sum(1)
                    one = minixr.Dataset({"v": (("time", "lat", "lon"), f)}, coords=ycoords)
                    out.append(pkg.weighted_aggregate_grid_to_regions_periods(one, "v", "popwt", "hierid", df, period="year"))
                return out

            a = call("record", "all")["tas-spell"].values
            ref = call("record", "referenced")["tas-spell"].values
            cut = call("period", "all")["tas-spell"].values
            b = np.stack([o["v"].values for o in per_threshold()])
            r = measure({"record_all": lambda: call("record", "all"), "record_referenced": lambda: call("record", "referenced"),
                         "period_all": lambda: call("period", "all"), "per_threshold": per_threshold}, sync, N_TIMED)
            both = np.isfinite(a) & np.isfinite(b)
            r["max_abs_diff_record_all_vs_per_threshold"] = float(np.abs(a - b)[both].max())
            r["max_abs_diff_record_referenced_vs_all"] = float(np.abs(ref - a)[np.isfinite(a) & np.isfinite(ref)].max())
            r["max_abs_diff_record_all_vs_period_all"] = float(np.abs(a - cut)[np.isfinite(a) & np.isfinite(cut)].max())
            r["nan_pattern_equal_record_all_vs_per_threshold"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
            r["mean_per_region_record_by_threshold"] = [round(float(v), 3) for v in np.nanmean(a, axis=(1, 2))]
            r["mean_per_region_period_by_threshold"] = [round(float(v), 3) for v in np.nanmean(cut, axis=(1, 2))]
            hot = hot_of(thresholds[0])
            ends = torch.arange(1, years, device="cuda") * DAYS_PER_YEAR
            r["share_of_cells_with_a_run_across_a_year_end_first_threshold"] = round(float((hot[ends - 1] & hot[ends]).any(0).float().mean()), 4)
            del hot
            for x, y in (("record_all", "per_threshold"), ("record_referenced", "per_threshold"), ("period_all", "record_all"),
                         ("record_all", "period_all"), ("record_all", "record_referenced"), ("record_referenced", "record_all")):
                r["%s_leads_%s" % (x, y)] = leads(r[x], r[y])
            res["%s_%s" % (dtype, cname)] = r
            print(dtype, cname, json.dumps(r), flush=True)
            dump()
        del ds, X
        pkg.clear_caches()
        torch.cuda.empty_cache()
    dump()
    print("wrote", path)


if __name__ == "__main__":
    main()
