#!/usr/bin/env python3
"""Annual totals (one period of T = 365 rows) of device-resident fields, per plan family: the two routes of
climate_toolbox_amd/periods.py against what a caller did before -- the daily apply followed by a sum over rows on the device.

  reduce_first     engine.period_reduce on X (T x G -> 1 x G), then the plan's apply on that one row
  aggregate_first  the plan's apply on the T rows, then engine.period_reduce (NaN kept) on the (T x R) result
  daily_then_sum   the plan's apply on the T rows, then a torch sum over dim 0 in fp64 (the code path before period totals)

Workloads: c2-real fp32 and c3 fp64 (segment table), c2-dense fp32 (full form, split kernel), a c5 block-local table
(tile-sparse).  Per variant: at least 0.3 s of warm-up, then the median of N >= 10 calls, each ending in a device
synchronise; the three variants of a workload alternate inside every round, so drift hits all of them alike.  The rule
the numbers are read by: a family's automatic route is reduce-first only if its median beats
aggregate-first by more than the larger of the two min-max spreads; neither route may be slower than daily_then_sum by
more than that spread.  Writes the JSON to the path given as the first argument (default profiles/period_timing.json).
``--only NAME`` runs one workload."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from climate_toolbox_amd import engine, synth  # noqa: E402

T, N_TIMED, WARM_S = 365, 12, 0.3


def measure(variants, sync):
    """{name: fn} -> {name: {"median_ms", "min_ms", "max_ms", "n"}}; warm-up per variant, then alternating rounds"""
    for fn in variants.values():
        t0 = time.perf_counter()
        while True:
            fn()
            sync()
            if time.perf_counter() - t0 >= WARM_S:
                break
    ts = {k: [] for k in variants}
    for _ in range(N_TIMED):
        for k, fn in variants.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}
            for k, v in ts.items()}


def workload(name, plan, X, torch):
    rb, rows = engine.period_lists([0, T], np.arange(T), T, device=X.device)
    dense = isinstance(plan, engine.DensePlan)
    apply = (lambda x: plan.apply(x)) if dense else (lambda x: plan.apply(x, layout="TG", out_layout="TR"))

    def reduce_first():
        field, status = engine.period_reduce(X, rb, rows, checked=True)
        out = apply(field[0])
        assert int(status.item()) == 0                  # (the public call reads the word too: it decides the fallback)
        return out

    def aggregate_first():
        return engine.period_reduce(apply(X), rb, rows, keep_nan=True, checked=True)[0][0]

    def daily_then_sum():
        return apply(X).sum(dim=0, dtype=torch.float64, keepdim=True).to(X.dtype)

    a, b, c = reduce_first().double(), aggregate_first().double(), daily_then_sum().double()
    scale = b.abs().clamp_min(1e-30)
    r = measure({"reduce_first": reduce_first, "aggregate_first": aggregate_first, "daily_then_sum": daily_then_sum}, torch.cuda.synchronize)
    r["max_rel_diff_reduce_vs_aggregate"] = float(((a - b).abs() / scale).max())
    r["max_rel_diff_aggregate_vs_daily_sum"] = float(((b - c).abs() / scale).max())
    spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in ("reduce_first", "aggregate_first"))
    r["spread_ms"] = round(spread, 4)
    r["auto_route"] = "reduce_first" if r["aggregate_first"]["median_ms"] - r["reduce_first"]["median_ms"] > spread else "aggregate_first"
    r["slower_than_daily_then_sum"] = [k for k in ("reduce_first", "aggregate_first")
                                       if r[k]["median_ms"] - r["daily_then_sum"]["median_ms"] > spread]
    r["family"] = "dense (form %d)" % plan.info["form"] if dense else "segment table"
    print(name, json.dumps(r), flush=True)
    return r


def main():
    import torch
    args = sys.argv[1:]
    only = args[args.index("--only") + 1] if "--only" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "period_timing.json")
    lat, lon, df = synth.realistic_segments()
    G = len(lat) * len(lon)
    res = {"T": T, "periods": 1, "G": G, "timed_calls": N_TIMED, "warm_up_s": WARM_S,
           "what": "annual total of a device-resident (365 x G) field; ms per call, host clock around a device synchronise"}
    jobs = [("c2-real fp32", "float32", "popwt"), ("c3 fp64", "float64", "popwt"), ("c2-dense fp32", "float32", None),
            ("c5-block fp32", "float32", None)]
    for name, dtype, wt in jobs:
        if only and not name.startswith(only):
            continue
        X = engine.synth_field(T, G, seed=11, base=280.0, amp=60.0, dtype=dtype)
        if wt is not None:
            cell, code, w, _ = synth.code_segments(df, lat, lon, "areawt" if name.startswith("c2") else wt, "hierid")
            plan = engine.SparsePlan(cell, code, w, G, int(code.max()) + 1, row_len=len(lon))
        elif name.startswith("c2-dense"):
            plan = engine.DensePlan.synth(G, 24378, seed=2)
        else:
            plan = engine.DensePlan.synth_blocklocal(G, 24378, seed=2)
        res[name] = workload(name, plan, X, torch)
        plan.close()
        del X
        torch.cuda.empty_cache()
    fam = {"segment": [k for k in ("c2-real fp32", "c3 fp64") if k in res], "dense": [k for k in ("c2-dense fp32", "c5-block fp32") if k in res]}
    res["reduce_first_families"] = sorted(f for f, ks in fam.items() if ks and all(res[k]["auto_route"] == "reduce_first" for k in ks))
    with open(path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
