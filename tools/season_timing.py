#!/usr/bin/env python3
"""Growing-season annual totals at c2-real shape (T = 365, 720 x 1440 cells; fp32 and fp64), device-resident, with a synthetic
window field of 150-day seasons whose start varies smoothly with latitude (wrapping the year end in the south):

  season_real      engine.season_reduce with those windows: pieces of rows out of season are not loaded
  season_open      engine.season_reduce with every window open all year: the same bytes as the period kernel
  period           engine.period_reduce on the same field -- the existing kernel, the yardstick
  call_season      weighted_aggregate_grid_to_regions_periods(..., period="year", season=windows), device-resident dataset
  host_premasked   what a caller had to do before: mask the materialised field on the host in NumPy, then
                   weighted_aggregate_grid_to_regions_periods on the host-resident result (few calls: seconds each)

Per variant: at least 0.3 s of warm-up, then N calls, each ending in a device synchronise; the three kernel variants alternate
inside every round, so drift hits all of them alike.  Reported: median, min, max in ms and, for the kernels, the bytes the
kernel asks for (16-byte pieces actually loaded, windows, days, the result) over the median against the 8 TB/s HBM peak.
The two things to read off: does season_open stay within the larger min-max spread of period, and does
season_real beat season_open.  Writes the JSON to the path given as the first argument (default profiles/season_timing.json);
``--only float32`` / ``--only float64`` runs one element type, ``--no-host`` skips host_premasked."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import climate_toolbox_amd as pkg  # noqa: E402
from climate_toolbox_amd import engine, minixr, synth  # noqa: E402

T, N_TIMED, N_HOST, WARM_S, PEAK = 365, 12, 3, 0.3, 8e12


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def measure(variants, sync, n, warm_s=WARM_S):
    """{name: fn} -> {name: stats}; warm-up per variant, then alternating rounds"""
    for fn in variants.values():
        t0 = time.perf_counter()
        while True:
            fn()
            sync()
            if time.perf_counter() - t0 >= warm_s:
                break
    ts = {k: [] for k in variants}
    for _ in range(n):
        for k, fn in variants.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    return {k: stats(v) for k, v in ts.items()}


def growing_days(lat, lon):
    """150-day seasons: the first day moves smoothly with latitude, half a year apart between the hemispheres"""
    start = (120.0 + 183.0 * (lat < 0) + 40.0 * np.sin(np.deg2rad(lat) * 3)) % 365.0 + 1.0
    end = start + 149.0
    z1 = np.repeat(np.floor(start)[:, None], len(lon), axis=1)
    z2 = np.repeat(np.floor(np.where(end > 365.0, end - 365.0, end))[:, None], len(lon), axis=1)
    return minixr.Dataset({"variable": (("z", "latitude", "longitude"), np.stack([z1, z2]))},
                          coords={"z": np.array([1, 2]), "latitude": lat, "longitude": lon + 180.0})


def in_season(win, doy):
    """(T, n) bool from the packed windows (include/wagg.h)"""
    w, d = win[None, :].astype(np.int64), doy[:, None].astype(np.int64)
    inside = (d >= (w & 1023)) & (d <= ((w >> 10) & 1023))
    return (inside != ((w >> 20) & 1).astype(bool)) & (((w >> 21) & 1) == 0)


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "season_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    sw = pkg.season_windows(growing_days(lat, lon))
    win = np.ascontiguousarray(sw.windows.reshape(-1))
    time_values = np.datetime64("2001-01-01") + np.arange(T)
    doy = pkg.day_of_year(time_values)
    mask = in_season(win, doy)                                                    # (T, G)
    res = {"T": T, "G": G, "periods": 1, "timed_calls": N_TIMED, "timed_calls_host_premasked": N_HOST, "warm_up_s": WARM_S,
           "in_season_share": round(float(mask.mean()), 4), "hbm_peak_bytes_per_s": PEAK,
           "what": "annual growing-season total of a device-resident (365 x G) field; ms per call, host clock around a device synchronise"}
    sync = torch.cuda.synchronize
    for dtype in ("float32", "float64"):
        if only and dtype != only:
            continue
        X = engine.synth_field(T, G, seed=11, base=280.0, amp=60.0, dtype=dtype)
        es = X.element_size()
        vec = 16 // es
        rb, rw = engine.period_lists([0, T], np.arange(T), T, device=X.device)
        doy_d = torch.from_numpy(doy).to(X.device)
        win_d = torch.from_numpy(win).to(X.device)
        open_d = torch.full((G,), 1023 << 10, dtype=torch.int32, device=X.device)
        kernels = {"season_real": lambda: engine.season_reduce(X, rb, rw, doy_d, win_d, checked=True),
                   "season_open": lambda: engine.season_reduce(X, rb, rw, doy_d, open_d, checked=True),
                   "period": lambda: engine.period_reduce(X, rb, rw, checked=True)}
        a, b, c = (kernels[k]()[0].double() for k in ("season_real", "season_open", "period"))
        r = measure(kernels, sync, N_TIMED)
        sub = np.arange(0, G, 7)                                                  # (the check, on every seventh cell)
        want = torch.from_numpy((X[:, ::7].cpu().numpy().astype(np.float64) * mask[:, sub]).sum(axis=0)).to(X.device)
        r["season_open_bit_equal_to_period"] = bool(torch.equal(b, c))
        r["season_real_max_rel_diff_vs_numpy"] = float(((a[0, 0, ::7] - want).abs() / want.abs().clamp_min(1e-30)).max())
        pieces = int(mask.reshape(T, G // vec, vec).any(axis=2).sum())
        out_b = G * es
        req = {"season_real": pieces * 16 + 4 * G + 4 * T + out_b, "season_open": T * G * es + 4 * G + 4 * T + out_b, "period": T * G * es + out_b}
        for k, nbytes in req.items():
            r[k]["bytes_requested"] = nbytes
            r[k]["bytes_per_s"] = round(nbytes / (r[k]["median_ms"] * 1e-3))
            r[k]["share_of_hbm_peak"] = round(nbytes / (r[k]["median_ms"] * 1e-3) / PEAK, 4)
        spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in ("season_open", "period"))
        r["spread_ms"] = round(spread, 4)
        r["open_minus_period_ms"] = round(r["season_open"]["median_ms"] - r["period"]["median_ms"], 4)
        r["open_within_spread_of_period"] = bool(r["open_minus_period_ms"] <= spread)
        r["real_minus_open_ms"] = round(r["season_real"]["median_ms"] - r["season_open"]["median_ms"], 4)
        r["skipping_loads_wins"] = bool(-r["real_minus_open_ms"] > max(spread, r["season_real"]["max_ms"] - r["season_real"]["min_ms"]))
        # the public call, device-resident
        field = X.reshape(T, len(lat), len(lon))
        ds = minixr.Dataset({"tas": (("time", "lat", "lon"), field)}, coords={"time": time_values, "lat": lat, "lon": lon})
        call = lambda: pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "hierid", df, period="year", season=sw)
        got = call().tas.values
        r.update(measure({"call_season": call}, sync, N_TIMED))
        if "--no-host" not in args:
            Xh = X.cpu().numpy().reshape(T, len(lat), len(lon))
            m3 = mask.reshape(Xh.shape)

            def host_premasked():
                pre = np.where(m3, Xh, Xh.dtype.type(0))
                hds = minixr.Dataset({"tas": (("time", "lat", "lon"), pre)}, coords={"time": time_values, "lat": lat, "lon": lon})
                return pkg.weighted_aggregate_grid_to_regions_periods(hds, "tas", "popwt", "hierid", df, period="year")

            old = host_premasked().tas.values
            r.update(measure({"host_premasked": host_premasked}, sync, N_HOST, warm_s=0.0))
            fin = np.isfinite(old)
            r["call_season_max_rel_diff_vs_host_premasked"] = float((np.abs(got - old)[fin] / np.maximum(np.abs(old[fin]), 1e-30)).max())
            r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(got), np.isnan(old)))
            del Xh, m3
        res[dtype] = r
        print(dtype, json.dumps(r), flush=True)
        del X, field, ds
        pkg.clear_caches()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
