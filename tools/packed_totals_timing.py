#!/usr/bin/env python3
"""``cells="referenced"`` against ``cells="all"``: annual totals of a 41-step degree-day ladder (0 .. 40 C) at c2-real shape
(T = 365, 720 x 1440 cells, the synthetic impact-region table; fp32 and fp64) through the public call
``snyder_edd_aggregate(..., period="year")``, with the synthetic 150-day season windows of tools/season_timing.py ("season")
and without a season ("allyear"), on device-resident fields ("device") and on host-resident ones ("host").

The two arms run in the same process and alternate inside every round:

  all         the whole grid is summed (a host-resident field uploaded whole): the code path as it was before 0.9.0
  referenced  the fields are packed to the quads the table references (host threads + PCIe of the packed rows only for a
              host-resident field, the pack kernel for a device-resident one), summed with n = Gq, contracted compact

Per arm: one warm-up call at least (0.3 s), then 12 timed calls, each ending in a device synchronise; reported as median, min
and max in ms.  Reported separately: the pack kernel alone on the device-resident pair of fields (``pack_kernel``), the packed
bytes that crossed PCIe in one host-resident call (``lines_h2d_bytes``, of ``field_bytes``), the way the packs went
(``pack_stats``), and the largest relative difference between the two arms' results.  Both arms include what the public call
does around the route: the label join, and the tasmin <= tasmax check, which uploads a host-resident pair whole in either arm.

The rule for a later change of the default (the one ``periods.REDUCE_FIRST_FAMILIES`` names): "referenced" becomes automatic for
a residency only if its median is ahead of "all" by more than the larger min-max spread of the two (``referenced_wins``).
Writes the JSON to the path given as the first argument (default profiles/packed_totals_timing.json) after every case;
``--only float32`` / ``--only float64`` runs one element type, ``--no-host`` leaves the host-resident cases out."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import _lib, _plans, engine, minixr, synth  # noqa: E402
from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, snyder_edd_aggregate  # noqa: E402
from season_timing import growing_days, measure  # noqa: E402

T, N_TIMED = 365, 12
LADDER = [float(e) for e in range(0, 41)]


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "packed_totals_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    res = {"T": T, "G": G, "periods": 1, "thresholds": LADDER, "timed_calls": N_TIMED, "warm_up_s": 0.3,
           "what": "snyder_edd_aggregate(period='year') of a 41-step ladder, cells='referenced' against cells='all'; ms per call, host "
                   "clock around a device synchronise"}
    sync = torch.cuda.synchronize

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        Xd = engine.synth_field(T, G, seed=11, base=287.0, amp=50.0, dtype=dtype)
        Hd = Xd + engine.synth_field(T, G, seed=12, base=9.0, amp=10.0, dtype=dtype)
        for residency in ("device", "host"):
            if residency == "host" and "--no-host" in args:
                continue
            if residency == "device":
                lo, hi = Xd.reshape(T, len(lat), len(lon)), Hd.reshape(T, len(lat), len(lon))
            else:
                lo, hi = Xd.cpu().numpy().reshape(T, len(lat), len(lon)), Hd.cpu().numpy().reshape(T, len(lat), len(lon))
            ds = minixr.Dataset({"tasmin": (("time", "lat", "lon"), lo), "tasmax": (("time", "lat", "lon"), hi)},
                                coords={"time": time_values, "lat": lat, "lon": lon})
            for k in ("tasmin", "tasmax"):
                ds[k].attrs["units"] = "K"
                ds = convert_kelvin_to_celsius(ds, k)
            for wname, season in (("season", sw), ("allyear", None)):
                call = lambda cells: snyder_edd_aggregate(ds, LADDER, "popwt", "hierid", df, period="year", season=season, cells=cells)
                before = dict(engine.PACK_STATS)
                _lib.host_stats(reset=True)
                got = call("referenced")["edd"].values
                h2d = _lib.host_stats()["lines_h2d_bytes"]
                went = {k: engine.PACK_STATS[k] - before[k] for k in before}
                old = call("all")["edd"].values
                r = measure({"all": lambda: call("all"), "referenced": lambda: call("referenced")}, sync, N_TIMED)
                fin = np.isfinite(old) & np.isfinite(got)
                r["max_rel_diff_referenced_vs_all"] = float((np.abs(got - old)[fin] / np.maximum(np.abs(old[fin]), 1e-30)).max())
                r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(got), np.isnan(old)))
                r["pack_stats"] = went
                r["lines_h2d_bytes"] = int(h2d)
                r["field_bytes"] = int(2 * T * G * Xd.element_size())
                spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in ("all", "referenced"))
                r["spread_ms"] = round(spread, 4)
                r["all_minus_referenced_ms"] = round(r["all"]["median_ms"] - r["referenced"]["median_ms"], 4)
                r["referenced_wins"] = bool(r["all_minus_referenced_ms"] > spread)
                key = "%s_%s_%s" % (dtype, residency, wname)
                res[key] = r
                print(key, json.dumps(r), flush=True)
                dump()
            if residency == "device":
                plan = [p for p in _plans._PLAN_CACHE.values() if isinstance(p, engine.SparsePlan)][-1]
                cells = plan.compact_cells(dtype)
                r = measure({"pack_kernel": lambda: engine.pack_rows(plan, Xd, Hd)}, sync, N_TIMED)
                r["Gq"] = int(len(cells))
                r["packed_share_of_row"] = round(len(cells) / G, 4)
                r["packed_bytes"] = int(2 * T * len(cells) * Xd.element_size())
                res["%s_pack" % dtype] = r
                print(dtype, "pack", json.dumps(r), flush=True)
                dump()
            del ds, lo, hi
        del Xd, Hd
        pkg.clear_caches()
        torch.cuda.empty_cache()
    dump()
    print("wrote", path)


if __name__ == "__main__":
    main()
