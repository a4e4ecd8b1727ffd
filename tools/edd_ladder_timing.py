#!/usr/bin/env python3
"""A 41-step degree-day ladder (0 .. 40 C) of annual totals at c2-real shape (T = 365, 720 x 1440 cells; fp32 and fp64),
device-resident Kelvin fields, with the synthetic 150-day season windows of tools/season_timing.py ("real") and with every
window open all year ("open").  Two kinds of field:

  noise     every cell drawn on its own: tasmin over 50 K around 287 K, tasmax 4 .. 14 K above it.  The 256 neighbouring cells
            a wave reads span every threshold, so the kernel's wave-level skip of the band expression is never taken
            (keys ``<dtype>_<windows>``)
  smooth    a field with the coherence of a daily temperature map: tasmin falls from the equator to the poles, swings with the
            season (opposite in the two hemispheres) and carries a slow wave along the longitude; the diurnal range is 5 .. 13 K
            and as smooth.  Neighbouring cells differ by a fraction of a kelvin, so a wave spans about a dozen of the 41
            thresholds and skips the rest (keys ``<dtype>_<windows>_smooth``)

The two legs:

  ladder    one engine.edd_ladder_reduce: all 41 planes in one launch
  grouped   the same planes from eleven engine.season_reduce calls of up to four thresholds -- the existing kernel, unchanged,
            in the same process: the yardstick

Per leg: at least 0.3 s of warm-up, then N timed repeats, each ending in a device synchronise; the two legs alternate inside
every round, so drift hits both alike.  Reported: median, min, max in ms per leg, whether the planes are bit-equal, and the
verdict the project asks for: the ladder's median must not exceed the grouped calls' median by more than the larger min-max
spread of the two legs.  Writes the JSON to the path given as the first argument (default profiles/edd_ladder_timing.json);
``--only float32`` / ``--only float64`` runs one element type."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import engine, synth  # noqa: E402
from season_timing import growing_days, measure  # noqa: E402

T, N_TIMED, KELVIN = 365, 12, -273.15
LADDER = [float(e) for e in range(0, 41)]


def smooth_fields(torch, lat, nlon, dtype):
    """(tasmin, tasmax) in kelvin as (T, nlat * nlon) device tensors: see the module docstring"""
    f8 = dict(dtype=torch.float64, device="cuda")
    t = torch.arange(T, **f8)[:, None, None]
    phi = torch.deg2rad(torch.as_tensor(np.asarray(lat, dtype=np.float64), device="cuda"))[None, :, None]
    lam = (2 * np.pi / nlon) * torch.arange(nlon, **f8)[None, None, :]
    year = 2 * np.pi * (t - 200.0) / 365.0
    lo = 273.15 - 12.0 + 27.0 * torch.cos(phi) + 9.0 * torch.sin(phi) * torch.cos(year) + 2.0 * torch.sin(3 * lam + t / 9.0)
    hi = lo + 9.0 + 4.0 * torch.cos(2 * lam + t / 30.0) * torch.cos(phi)
    dt = getattr(torch, dtype)
    return lo.reshape(T, -1).to(dt), hi.reshape(T, -1).to(dt)


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "edd_ladder_timing.json")
    lat, lon, _ = synth.realistic_segments()
    G = len(lat) * len(lon)
    win = np.ascontiguousarray(pkg.season_windows(growing_days(lat, lon)).windows.reshape(-1))
    doy = pkg.day_of_year(np.datetime64("2001-01-01") + np.arange(T))
    res = {"T": T, "G": G, "periods": 1, "thresholds": LADDER, "timed_repeats": N_TIMED, "warm_up_s": 0.3,
           "what": "annual totals of a 41-step degree-day ladder of device-resident (365 x G) fields; ms per leg, host clock around "
                   "a device synchronise; grouped = eleven engine.season_reduce calls of up to four thresholds"}
    sync = torch.cuda.synchronize
    groups = [LADDER[k:k + 4] for k in range(0, len(LADDER), 4)]
    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        for fname in ("noise", "smooth"):
            if fname == "noise":
                X = engine.synth_field(T, G, seed=11, base=287.0, amp=50.0, dtype=dtype)
                H = X + engine.synth_field(T, G, seed=12, base=9.0, amp=10.0, dtype=dtype)
            else:
                X, H = smooth_fields(torch, lat, len(lon), dtype)
            rb, rw = engine.period_lists([0, T], np.arange(T), T, device=X.device)
            doy_d = torch.from_numpy(doy).to(X.device)
            for wname, w in (("real", torch.from_numpy(win).to(X.device)),
                             ("open", torch.full((G,), 1023 << 10, dtype=torch.int32, device=X.device))):
                ladder = lambda: engine.edd_ladder_reduce(X, H, rb, rw, KELVIN, LADDER, doy=doy_d, windows=w, checked=True)[0]
                grouped = lambda: [engine.season_reduce(X, rb, rw, doy_d, w, X2=H, edd=(KELVIN, g), checked=True)[0] for g in groups]
                a, b = ladder(), torch.cat(grouped())
                r = measure({"ladder": ladder, "grouped": grouped}, sync, N_TIMED)
                r["field"] = fname
                r["bit_equal"] = bool(torch.equal(a, b))
                r["total_degree_days_mean"] = float(a.double().mean())
                spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in ("ladder", "grouped"))
                r["spread_ms"] = round(spread, 4)
                r["ladder_minus_grouped_ms"] = round(r["ladder"]["median_ms"] - r["grouped"]["median_ms"], 4)
                r["ladder_over_grouped"] = round(r["ladder"]["median_ms"] / r["grouped"]["median_ms"], 4)
                r["ladder_within_spread_of_grouped"] = bool(r["ladder_minus_grouped_ms"] <= spread)
                key = "%s_%s" % (dtype, wname) + ("" if fname == "noise" else "_smooth")
                res[key] = r
                print(key, json.dumps(r), flush=True)
                del a, b
            del X, H
            torch.cuda.empty_cache()
    res["ladder_never_slower"] = all(v["ladder_within_spread_of_grouped"] for v in res.values() if isinstance(v, dict))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
