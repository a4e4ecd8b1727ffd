#!/usr/bin/env python3
"""{popwt, areawt} x {hierid, ISO} of the c2-real table (fp32) and of c3 (fp64), T = 365: one many-plan call
(engine.ManyPlan: both weightings, ISO derived from the hierid partial sums) against the four single-plan calls, for a
host-resident field (HOST_PIN | HOST_LINES) and for a device-resident one.  Median of 7 after 2 warm-up calls; prints one
JSON object (and writes it to the path given as the first argument, if any).  ``--once``: one device apply of the
K = 2 many-plan (with ISO derived) and one of the single plan per data type, nothing else -- for a counter run (FETCH_SIZE)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from climate_toolbox_amd import _lib, engine, synth  # noqa: E402


def med(fn, n=7, warm=2, sync=None):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    import torch
    once = "--once" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--once"]
    lat, lon, df = synth.realistic_segments()
    cell, hier, pop, _ = synth.code_segments(df, lat, lon, "popwt", "hierid")
    _, _, area, _ = synth.code_segments(df, lat, lon, "areawt", "hierid")
    _, iso, _, iso_u = synth.code_segments(df, lat, lon, "areawt", "ISO")
    G, R, R_iso, T = len(lat) * len(lon), int(hier.max()) + 1, len(iso_u), 365
    flags = _lib.HOST_PIN | _lib.HOST_LINES
    res = {"T": T, "G": G, "R_hierid": R, "R_ISO": R_iso}
    for name, dtype in (("c2-real fp32", "float32"), ("c3 fp64", "float64")):
        X = engine.synth_field(T, G, seed=11, base=280.0, amp=60.0, dtype=dtype)
        Xh = X.cpu().numpy()
        many = engine.ManyPlan(cell, hier, [pop, area], G, R, row_len=len(lon), levels=[(iso, R_iso)])
        if once:
            single = engine.SparsePlan(cell, hier, pop, G, R, row_len=len(lon))
            many.apply(X); single.apply(X)
            torch.cuda.synchronize()
            many.close(); single.close()
            continue
        singles = [engine.SparsePlan(cell, c, w, G, r, row_len=len(lon)) for w in (pop, area) for c, r in ((hier, R), (iso, R_iso))]
        sync = torch.cuda.synchronize
        r = {"host_many_ms": med(lambda: many.apply_host(Xh, flags=flags)),
             "host_one_single_ms": med(lambda: singles[0].apply_host(Xh, flags=flags)),
             "host_four_single_ms": med(lambda: [s.apply_host(Xh, flags=flags) for s in singles]),
             "device_many_ms": med(lambda: many.apply(X), sync=sync),
             "device_four_single_ms": med(lambda: [s.apply(X) for s in singles], sync=sync)}
        r["host_many_over_one_single"] = r["host_many_ms"] / r["host_one_single_ms"]
        r["host_many_over_four"] = r["host_many_ms"] / r["host_four_single_ms"]
        r["device_many_over_four"] = r["device_many_ms"] / r["device_four_single_ms"]
        res[name] = r
        many.close()
        for s in singles:
            s.close()
    out = json.dumps(res, indent=1)
    print(out)
    if args:
        with open(args[0], "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
