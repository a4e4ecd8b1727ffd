#!/usr/bin/env python3
"""SHA-256 of the results of a fixed matrix of segment-table applies, one line per case and one digest over all of them.

The segment-table kernels use no atomics, so a build that sends every case to the same kernels gives the same bits: run on
two builds, equal output means no route changed between them.  Only the public Python surface is used (engine.SparsePlan,
engine.ManyPlan, engine.pack_rows), on the tables and fields of tests/test_gpu_fallback_routes.py:

  routes A-F x grids 40 x 36 and the ragged 37 x 27 x T in {1, 65} x fp32 / fp64 x both layouts x both result layouts x
  {plain, powers 1..3, powers 1..5, degree days at 1, 3, 6 thresholds}; packed rows (WAGG_APPLY_COMPACT_ROWS) on route F;
  a many-plan of two weightings with one derived level; apply_host in its plain row pipeline.

    python tools/route_bits.py [--out FILE]      (needs the GPU; seconds)
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the lines there as well")
    args = ap.parse_args()
    import torch
    from climate_toolbox_amd import engine
    from tests import test_gpu_fallback_routes as F

    lines, total = [], hashlib.sha256()

    def note(name, result):
        a = np.ascontiguousarray(result.cpu().numpy() if hasattr(result, "cpu") else result)
        h = hashlib.sha256(a.tobytes()).hexdigest()
        total.update(("%s %s %s\n" % (name, a.shape, h)).encode())
        lines.append("%s %s %s" % (name, "x".join(map(str, a.shape)), h))

    grids = [(40, 36), F.RAGGED]
    for grid in grids:
        t = F._table(*grid)
        gname = "%dx%d" % grid
        for route in ("A", "B", "C", "D", "EC", "ED", "F"):
            row_len, flags = F._route_args(route, t.nlon)
            plan = engine.SparsePlan(t.cell, t.code, t.w, t.G, t.R, row_len=row_len, flags=flags)
            for T in (1, 65):
                for dtype in (np.float32, np.float64):
                    X = np.array(F._field(*grid, dtype, T))
                    lo, hi = (np.array(a) for a in F._edd_fields(*grid, dtype, T))
                    dev = {"TG": [torch.from_numpy(a).cuda() for a in (X, lo, hi)],
                           "GT": [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (X, lo, hi)]}
                    for layout in ("TG", "GT"):
                        x, dlo, dhi = dev[layout]
                        for ol in ("TR", "RT"):
                            tag = "%s %s T%d %s %s %s" % (route, gname, T, np.dtype(dtype).name, layout, ol)
                            note(tag + " plain", plan.apply(x, layout=layout, out_layout=ol))
                            for K in (3, 5):
                                note(tag + " poly%d" % K, plan.apply_poly(x, F.OFFSET, K, layout=layout, out_layout=ol))
                            for k, thr in sorted(F.THRESHOLDS.items()):
                                note(tag + " edd%d" % k, plan.apply_edd(dlo, dhi, thr, offset=0.0, layout=layout, out_layout=ol))
                    if route == "F" and plan.compact_cells(dtype) is not None:
                        packed = engine.pack_rows(plan, dev["TG"][0])
                        note("F %s T%d %s compact" % (gname, T, np.dtype(dtype).name), plan.apply(packed, compact=True))
                    if route in ("A", "F"):
                        note("%s %s T%d %s apply_host" % (route, gname, T, np.dtype(dtype).name), plan.apply_host(X))
            plan.close()
        # two weightings, one derived level (four fine regions to a coarse one; null labels stay null)
        w2 = np.where(np.isnan(t.w), np.nan, 0.5 * t.w + 0.125)
        coarse = np.where(t.code < 0, -1, t.code // 4).astype(np.int32)
        many = engine.ManyPlan(t.cell, t.code, [t.w, w2], t.G, t.R, row_len=t.nlon if t.nlon % 4 == 0 else 0,
                               levels=[(coarse, (t.R + 3) // 4)] if t.nlon % 4 == 0 else ())
        for T in (1, 65):
            for dtype in (np.float32, np.float64):
                x = torch.from_numpy(np.array(F._field(*grid, dtype, T))).cuda()
                for ol in ("TR", "RT"):
                    out = torch.empty((T, many.out_cols) if ol == "TR" else (many.out_cols, T), dtype=x.dtype, device="cuda")
                    many.apply(x, out_layout=ol, out=out)
                    note("many %s T%d %s TG %s" % (gname, T, np.dtype(dtype).name, ol), out)
        many.close()
    torch.cuda.synchronize()
    lines.append("total %d %s" % (len(lines), total.hexdigest()))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
        print(lines[-1])
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
