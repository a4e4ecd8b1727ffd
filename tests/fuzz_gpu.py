#!/usr/bin/env python3
"""Randomised differential run of every C-ABI compute entry point against the oracle (GPU box).
usage: python tests/fuzz_gpu.py [n_cases] [seed]      -- prints one line per failing case, exit 1 on any
FUZZ_LINES=1: lines_case (the lines-only host path); FUZZ_MANY=1: many_case (many-plans, wagg_plan_create_many);
FUZZ_FLAGS=1: flags_case (the kernels behind the WAGG_PLAN_NO_* flags and plans without a row length);
FUZZ_FORMS=1: forms_case (dense-family plans with a forced form: full, tile-sparse, entry lists);
FUZZ_BUILD=1: build_case (the device plan builder: every stored weight against the table-order pair sum);
FUZZ_ELEMENTS=1: elements_case (relayout, to_float64, take_axis, gather: bits against tests/element_ops.py);
FUZZ_SPLIT=1: split_case (the split form of fp32 full-form plans under power-of-two row and column scales)"""
import os, sys, traceback
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from climate_toolbox_amd.engine import SparsePlan, DensePlan
from oracle import ref_numpy as O

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
SEED = int(sys.argv[2]) if len(sys.argv) > 2 else 0


N_LINES = 0
N_FUSED = 0


def rel_bad(got, ref, rtol, scale):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return "shape %r vs %r" % (got.shape, ref.shape)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return "NaN pattern differs at %d places" % (np.isnan(got) != np.isnan(ref)).sum()
    fin = np.isfinite(ref)
    inf = ~fin & ~np.isnan(ref)
    if not np.array_equal(got[inf], ref[inf]):
        return "inf values differ"
    err = np.abs(got[fin] - ref[fin])
    tol = rtol * np.maximum(np.abs(ref[fin]), scale)
    if (err > tol).any():
        return "max err/tol %.3g" % (err / tol).max()
    return None


def edge_thresholds(thr, lo, hi, cell, off, dtype):
    """``thr`` and, in about a third of the cases, one or two more thresholds that EQUAL ``dtype(tasmin + off)`` or
    ``dtype(tasmax + off)`` of a cell the table references: the band edges, where the reference selects M - e or 0.  The draw
    comes from a generator of its own (seeded by the case's first threshold), and the thresholds are appended: a seed's case is
    what it was, with at most two planes more."""
    if not len(cell) or not lo.size:
        return thr
    side = np.random.default_rng(int(abs(thr[0]) * 1e9) % (1 << 32))
    if side.random() >= 0.35:
        return thr
    more = []
    for _ in range(int(side.integers(1, 3))):
        t, c = int(side.integers(0, lo.shape[0])), int(cell[int(side.integers(0, len(cell)))])
        v = float(dtype((lo if side.random() < 0.5 else hi)[t, c] + dtype(off)))
        if np.isfinite(v):
            more.append(v)
    return thr + more


def one_case(i, rng):
    dtype = np.float32 if rng.random() < 0.6 else np.float64
    rtol = 1e-4 if dtype == np.float32 else 1e-6
    T = int(rng.choice([1, 2, 3, 7, 16, 63, 64, 65, 100, 129, 200, 366]))
    sc = int(os.environ.get("FUZZ_SCALE", "1"))                                        # larger grids on request
    nlat, nlon = int(rng.integers(1, 60 * sc)), int(rng.integers(1, 90 * sc))
    G = nlat * nlon
    R = int(rng.integers(1, 300))
    nseg = int(rng.integers(0, min(4 * G, 400000) + 2))
    cell = rng.integers(0, G, nseg).astype(np.int32)
    code = rng.integers(-1 if rng.random() < 0.3 else 0, R, nseg).astype(np.int32)     # some null labels
    if rng.random() < 0.5:
        # a COMPACT table (regions = blocks of the grid with holes, a few split cells): what the whole-line chunkings
        # are built for -- a scattered table above is declined by them (too many partial rows)
        bh, bw = int(rng.integers(1, 9)), int(rng.integers(1, 17))
        keep = np.flatnonzero(rng.random(G) < rng.uniform(0.3, 1.0))
        nbw = (nlon + bw - 1) // bw
        reg = ((keep // nlon) // bh) * nbw + (keep % nlon) // bw
        R = int(reg.max()) + 1 + int(rng.integers(0, 3)) if len(keep) else R           # (sometimes a region nobody maps to)
        extra = rng.choice(keep, min(len(keep), 40)) if len(keep) else keep
        cell = np.concatenate([keep, extra]).astype(np.int32)
        code = np.concatenate([reg, rng.integers(0, R, len(extra))]).astype(np.int32)
        if rng.random() < 0.3 and len(code):
            code[rng.integers(0, len(code), 3)] = -1
    if rng.random() < 0.4 and G > 700:                                                # a giant region
        n = int(rng.integers(300, min(G, 3000)))
        cell = np.concatenate([cell, rng.choice(G, n, replace=False).astype(np.int32)])
        code = np.concatenate([code, np.zeros(n, np.int32)])
    w = rng.uniform(0.05, 3.0, len(cell))
    w[rng.random(len(cell)) < 0.05] = np.nan
    w[rng.random(len(cell)) < 0.03] = 0.0
    X = (288.0 + 9.0 * rng.standard_normal((T, G))).astype(dtype)
    if rng.random() < 0.5:
        X[rng.integers(0, T, 5), rng.integers(0, G, 5)] = np.nan
    if rng.random() < 0.2:
        X[rng.integers(0, T), rng.integers(0, G)] = np.inf
    layout = "TG" if rng.random() < 0.7 else "GT"
    out_layout = "TR" if rng.random() < 0.7 else "RT"
    pad = int(rng.choice([0, 0, 1, 3, 4]))                                            # row stride > G / unaligned rows
    tag = "case %d: %s T=%d grid=%dx%d R=%d nseg=%d %s->%s pad=%d" % (i, dtype.__name__, T, nlat, nlon, R, len(cell), layout, out_layout, pad)
    plan = SparsePlan(cell, code, w, G, R, row_len=nlon)
    ref = O.agg_coded(X, cell, code, w, R)
    def dev(a):                                                                       # optionally padded rows
        a = a if layout == "TG" else np.ascontiguousarray(a.T)
        if pad:
            buf = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.from_numpy(a).dtype, device="cuda")
            buf[:, :a.shape[1]] = torch.from_numpy(a).cuda()
            return buf[:, :a.shape[1]]
        return torch.from_numpy(a).cuda()
    Xd = dev(X)
    fails = []
    got = plan.apply(Xd, layout=layout, out_layout=out_layout).cpu().numpy()
    got = got if out_layout == "TR" else got.T
    b = rel_bad(got, ref, rtol, 1.0)
    if b: fails.append("apply: " + b)
    from climate_toolbox_amd import _lib
    host_forms = layout == "TG" and out_layout == "TR"
    hflags = int(rng.choice([0, _lib.HOST_PIN, _lib.HOST_LINES, _lib.HOST_PIN | _lib.HOST_LINES, _lib.HOST_PIN | _lib.HOST_LINES | _lib.HOST_LINES_WHOLE]))
    if host_forms:                                            # the host forms of the same call (row-block pipeline; lines only
        _lib.host_stats(reset=True)                           #  when the field is large enough -- FUZZ_SCALE >= 6 -- and compact)
        gh = plan.apply_host(X, flags=hflags)
        b = rel_bad(gh, ref, rtol, 1.0)
        if b: fails.append("apply_host(flags %d): %s" % (hflags, b))
        if pad == 0 and not np.array_equal(gh, got, equal_nan=True): fails.append("apply_host(flags %d) differs from the device apply" % hflags)
        if _lib.host_stats()["lines_h2d_bytes"]: tag += " [lines]"
    kind = rng.integers(0, 3)
    if kind == 0:                                                                     # fused powers
        K = int(rng.integers(1, 6))
        gp = plan.apply_poly(Xd, -273.15, K, layout=layout, out_layout=out_layout).cpu().numpy()
        for p in range(1, K + 1):
            g = gp[p - 1] if out_layout == "TR" else gp[p - 1].T
            # sums of signed powers cancel: the error is relative to the size of the terms
            # (|y| ~ 15 +- 9 here), so |ref| is floored at 10^p
            b = rel_bad(g, O.agg_coded(O.tas_poly_values(X, p), cell, code, w, R), rtol, 10.0 ** p)
            if b: fails.append("poly p=%d: %s" % (p, b))
        if host_forms:
            gph = plan.apply_poly_host(X, -273.15, K, flags=hflags)
            if pad == 0 and not np.array_equal(gph, gp, equal_nan=True): fails.append("apply_poly_host(flags %d) differs from the device form" % hflags)
            for p in range(1, K + 1):
                b = rel_bad(gph[p - 1], O.agg_coded(O.tas_poly_values(X, p), cell, code, w, R), rtol, 10.0 ** p)
                if b: fails.append("poly_host p=%d: %s" % (p, b))
    elif kind == 1:                                                                   # degree days
        half = rng.uniform(0, 8, X.shape).astype(dtype)
        lo, hi = X - half, X + half
        thr = [float(rng.uniform(5, 35)) for _ in range(int(rng.integers(1, 7)))]        # 1..6: passes of four + a rest
        thr = edge_thresholds(thr, lo, hi, cell, -273.15, dtype)
        ge = plan.apply_edd(dev(lo), dev(hi), thr, offset=-273.15, layout=layout, out_layout=out_layout).cpu().numpy()
        ft = dtype
        for k, e in enumerate(thr):
            g = ge[k] if out_layout == "TR" else ge[k].T
            b = rel_bad(g, O.agg_coded(O.snyder_edd_values(lo + ft(-273.15), hi + ft(-273.15), e), cell, code, w, R), rtol, 0.05)
            if b: fails.append("edd e=%.2f: %s" % (e, b))
        if host_forms:
            geh = plan.apply_edd_host(lo, hi, thr, offset=-273.15, flags=hflags)
            if pad == 0 and not np.array_equal(geh, ge, equal_nan=True): fails.append("apply_edd_host(flags %d) differs from the device form" % hflags)
            for k, e in enumerate(thr):
                b = rel_bad(geh[k], O.agg_coded(O.snyder_edd_values(lo + ft(-273.15), hi + ft(-273.15), e), cell, code, w, R), rtol, 0.05)
                if b: fails.append("edd_host e=%.2f: %s" % (e, b))
    elif layout == "TG" and not np.isinf(X).any():            # dense family: the library's choice of form, or one pinned
        form = [None, "full", "tiles", "entries"][int(rng.integers(0, 4))]              # (round 5: the choice goes by estimated
        dp = DensePlan.from_segments(cell, code, w, G, R, dtype=dtype, form=form)       #  time, so small tables mostly take entry
        b = rel_bad(dp.apply(Xd.contiguous()).cpu().numpy(), ref, rtol, 1.0)            #  lists by themselves: pin the others)
        fname = ["full", "tiled", "entries"][dp.info["form"]]
        if b: fails.append("dense(%s, asked %s): %s" % (fname, form, b))
        # a tall ragged batch of the same rows (full row blocks + a shorter remainder: two launches), and a cloned plan
        T2 = int(rng.choice([500, 700, 1369, 1500]))
        idx = rng.integers(0, T, T2)
        Xt = Xd.contiguous()[torch.from_numpy(idx).cuda()]
        gt = dp.apply(Xt).cpu().numpy()
        b = rel_bad(gt, ref[idx], rtol, 1.0)
        if b: fails.append("dense(%s) tall batch T=%d: %s" % (fname, T2, b))
        if rng.random() < 0.4:
            rep = dp.replica(0)
            if not np.array_equal(rep.apply(Xt).cpu().numpy(), gt, equal_nan=True): fails.append("dense(%s): the clone's result differs" % fname)
            rep.close()
        dp.close()
        if rng.random() < 0.5 and len(cell):
            # the same table as CSR (rows = cells, columns ascending): the one-pass sort when nothing is dropped
            order = np.lexsort((code, cell))
            rowptr = np.zeros(G + 1, np.int64)
            np.add.at(rowptr, cell[order].astype(np.int64) + 1, 1)
            dc = DensePlan.from_csr(np.cumsum(rowptr), code[order], w[order], G, R, dtype=dtype, form=form)
            want_one_pass = int(not ((code < 0).any() or np.isnan(w).any()) and dc.info["one_pass_sort"] == 1)
            b = rel_bad(dc.apply(Xt).cpu().numpy(), ref[idx], rtol, 1.0)
            if b: fails.append("dense from CSR (one pass: %d): %s" % (dc.info["one_pass_sort"], b))
            if dc.info["one_pass_sort"] and ((code < 0).any() or np.isnan(w).any()): fails.append("one-pass sort taken with dropped rows")
            dc.close()
    plan.close()
    return tag, fails


def lines_case(i, rng):
    """FUZZ_LINES=1: fields large and tables compact enough for the lines-only host path (land masks with coasts, random
    grids and land fractions): the three host forms with WAGG_HOST_LINES against the device forms of the same kernels, bit
    for bit, and against the oracle."""
    from climate_toolbox_amd import _lib, synth
    dtype = np.float32 if rng.random() < 0.6 else np.float64
    rtol = 1e-4 if dtype == np.float32 else 1e-6
    nlat, nlon = int(rng.integers(64, 200)), 4 * int(rng.integers(40, 160))
    G = nlat * nlon
    lat, lon, df = synth.realistic_segments(nlat=nlat, nlon=nlon, R=int(rng.integers(5, 900)), n_iso=5, seed=int(rng.integers(0, 1 << 30)),
                                            land_frac=float(rng.uniform(0.03, 0.35)), string_labels=False)
    cell, code, w, uniq = synth.code_segments(df, lat, lon, "popwt" if rng.random() < 0.5 else "areawt", "hierid")
    R = len(uniq)
    T = int(((64 << 20) // (G * np.dtype(dtype).itemsize) + 1) * rng.uniform(1.0, 1.6)) + int(rng.integers(0, 9))
    X = (288.0 + 9.0 * rng.standard_normal((T, G))).astype(dtype)
    X[rng.integers(0, T, 50), rng.integers(0, G, 50)] = np.nan
    if rng.random() < 0.3:
        X[rng.integers(0, T), cell[rng.integers(0, len(cell))]] = np.inf
    flags = _lib.HOST_LINES | (_lib.HOST_PIN if rng.random() < 0.7 else 0) | (_lib.HOST_LINES_WHOLE if rng.random() < 0.4 else 0)    # quads only / whole lines
    tag = "lines case %d: %s T=%d grid=%dx%d R=%d nseg=%d flags=%d" % (i, dtype.__name__, T, nlat, nlon, R, len(cell), flags)
    plan = SparsePlan(cell, code, w, G, R, row_len=nlon)
    fails = []
    Xd = torch.from_numpy(X).cuda()
    _lib.host_stats(reset=True)
    gh = plan.apply_host(X, flags=flags)
    took = _lib.host_stats()["lines_h2d_bytes"] > 0
    tag += " [lines]" if took else " [whole rows]"
    if not np.array_equal(gh, plan.apply(Xd).cpu().numpy(), equal_nan=True): fails.append("apply_host differs from the device apply")
    b = rel_bad(gh, O.agg_coded(X, cell, code, w, R), rtol, 1.0)
    if b: fails.append("apply_host: " + b)
    kind = int(rng.integers(0, 2))
    if kind == 0:
        K = int(rng.integers(1, 6))
        gp = plan.apply_poly_host(X, -273.15, K, flags=flags)
        if not np.array_equal(gp, plan.apply_poly(Xd, -273.15, K).cpu().numpy(), equal_nan=True): fails.append("apply_poly_host differs from the device form")
        b = rel_bad(gp[K - 1], O.agg_coded(O.tas_poly_values(X, K), cell, code, w, R), rtol, 10.0 ** K)
        if b: fails.append("poly_host p=%d: %s" % (K, b))
    else:
        half = rng.uniform(0, 8, X.shape).astype(dtype)
        lo, hi = X - half, X + half
        thr = [float(rng.uniform(5, 35)) for _ in range(int(rng.integers(1, 6)))]
        thr = edge_thresholds(thr, lo, hi, cell, -273.15, dtype)
        ge = plan.apply_edd_host(lo, hi, thr, offset=-273.15, flags=flags)
        gd = plan.apply_edd(torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda(), thr, offset=-273.15).cpu().numpy()
        if not np.array_equal(ge, gd, equal_nan=True): fails.append("apply_edd_host differs from the device form")
        b = rel_bad(ge[0], O.agg_coded(O.snyder_edd_values(lo + dtype(-273.15), hi + dtype(-273.15), thr[0]), cell, code, w, R), rtol, 0.05)
        if b: fails.append("edd_host e=%.2f: %s" % (thr[0], b))
    plan.close()
    return tag, fails


def many_case(i, rng):
    """FUZZ_MANY=1: many-plans (engine.ManyPlan) over compact tables: 1..4 weight columns with independent NaN / 0 entries,
    0..3 derived levels (the block coordinates integer-divided, so they nest by construction), sometimes a null label shared
    by all levels, NaN and sometimes +-inf data, padded / unaligned rows, either result layout.  Every plane against the
    oracle over that weighting's raw column, the fine planes bit for bit the single plans over the columns the many-plan
    uses; for unpadded (time, region) results one host flag set, bit for bit the device apply.  A table without the
    whole-line chunking of the data type must refuse derived levels; the case goes on with none."""
    from climate_toolbox_amd import _lib
    from climate_toolbox_amd.engine import ManyPlan
    dtype = np.float32 if rng.random() < 0.6 else np.float64
    rtol = 1e-4 if dtype == np.float32 else 1e-6
    T = int(rng.choice([1, 2, 3, 7, 16, 63, 64, 65, 100, 129, 200]))
    sc = int(os.environ.get("FUZZ_SCALE", "1"))
    nlat = int(rng.integers(2, 60 * sc))
    nlon = 4 * int(rng.integers(1, 23 * sc)) if rng.random() < 0.85 else int(rng.integers(1, 90 * sc))   # (whole-line chunkings: rows of whole quads)
    G = nlat * nlon
    # the compact table of one_case: regions = blocks of the grid with holes, a few split cells
    bh, bw = int(rng.integers(1, 9)), int(rng.integers(1, 17))
    keep = np.flatnonzero(rng.random(G) < rng.uniform(0.3, 1.0))
    if not len(keep):
        keep = np.array([int(rng.integers(0, G))])
    nbw = (nlon + bw - 1) // bw
    reg = ((keep // nlon) // bh) * nbw + (keep % nlon) // bw
    R = int(reg.max()) + 1 + int(rng.integers(0, 3))                                   # (sometimes a region nobody maps to)
    extra = rng.choice(keep, min(len(keep), 40))
    cell = np.concatenate([keep, extra]).astype(np.int32)
    code = np.concatenate([reg, rng.integers(0, R, len(extra))]).astype(np.int32)
    null = np.zeros(len(code), dtype=bool)
    if rng.random() < 0.4:
        null[rng.integers(0, len(code), 3)] = True
    L = int(rng.integers(0, 4))
    levels, f = [], 1
    for _ in range(L):                                                                 # block (by, bx) -> (by // f, bx // f)
        f *= int(rng.integers(2, 4))
        nbc = (nbw + f - 1) // f
        lc = ((code // nbw) // f) * nbc + (code % nbw) // f
        levels.append((np.where(null, -1, lc).astype(np.int32), (((R - 1) // nbw) // f + 1) * nbc + int(rng.integers(0, 2))))
    code[null] = -1
    K = int(rng.integers(1, 5))
    ws = []
    for _ in range(K):
        w = rng.uniform(0.05, 3.0, len(cell))
        w[rng.random(len(cell)) < 0.05] = np.nan
        w[rng.random(len(cell)) < 0.03] = 0.0
        ws.append(w)
    kept = ~np.isnan(np.stack(ws)).all(axis=0)
    cols = [np.where(kept, np.where(np.isnan(w), 0.0, w), np.nan) for w in ws]         # what the many-plan makes of column k
    X = (288.0 + 9.0 * rng.standard_normal((T, G))).astype(dtype)
    if rng.random() < 0.6:
        X[rng.integers(0, T, 5), cell[rng.integers(0, len(cell), 5)]] = np.nan
    if rng.random() < 0.4:
        X[rng.integers(0, T), cell[rng.integers(0, len(cell))]] = np.inf
    if rng.random() < 0.3:
        X[rng.integers(0, T), cell[rng.integers(0, len(cell))]] = -np.inf
    out_layout = "TR" if rng.random() < 0.6 else "RT"
    pad = int(rng.choice([0, 0, 1, 3, 4]))
    hflags = int(rng.choice([0, _lib.HOST_PIN, _lib.HOST_WHOLE, _lib.HOST_PIN | _lib.HOST_WHOLE, _lib.HOST_LINES, _lib.HOST_PIN | _lib.HOST_LINES,
                             _lib.HOST_PIN | _lib.HOST_LINES | _lib.HOST_LINES_WHOLE]))
    tag = "many case %d: %s T=%d grid=%dx%d R=%d nseg=%d K=%d L=%d TG->%s pad=%d" % (i, dtype.__name__, T, nlat, nlon, R, len(cell), K, L, out_layout, pad)
    if pad:
        buf = torch.full((T, G + pad), float("nan"), dtype=torch.from_numpy(X).dtype, device="cuda")
        c0 = 1 if pad in (1, 3) else 0                                                 # (pad 1, 3: rows that are not 16-byte aligned)
        buf[:, c0:c0 + G] = torch.from_numpy(X).cuda()
        Xd = buf[:, c0:c0 + G]
    else:
        Xd = torch.from_numpy(X).cuda()
    fails = []
    plan = ManyPlan(cell, code, ws, G, R, row_len=nlon, levels=levels)
    fused = bool(plan.info["lines"] & (1 if dtype == np.float32 else 2))
    if not fused and L:
        try:
            plan.apply(Xd, out_layout=out_layout)
            fails.append("derived levels without the whole-line chunking were not refused")
        except _lib.WaggError as e:
            if e.code != -5: fails.append("derived levels refused with code %d" % e.code)
        plan.close()
        levels, L = [], 0
        plan = ManyPlan(cell, code, ws, G, R, row_len=nlon)
    tag += " [fused]" if fused else " [one by one]"
    views = plan.apply(Xd, out_layout=out_layout)
    got = [[v.cpu().numpy() if out_layout == "TR" else v.cpu().numpy().T for v in row] for row in views]
    for l, (lc, Rl) in enumerate([(code, R)] + levels):
        for k in range(K):
            b = rel_bad(got[l][k], O.agg_coded(X, cell, lc, ws[k], Rl), rtol, 1.0)
            if b: fails.append("plane (%d, %d): %s" % (l, k, b))
    for k in range(K):
        single = SparsePlan(cell, code, cols[k], G, R, row_len=nlon)
        g1 = single.apply(Xd, out_layout=out_layout).cpu().numpy()
        if not np.array_equal(g1 if out_layout == "TR" else g1.T, got[0][k], equal_nan=True): fails.append("fine plane %d differs from the single plan" % k)
        if not np.array_equal(plan.den[0][k], single.den, equal_nan=True): fails.append("den of weighting %d differs from the single plan" % k)
        single.close()
    if pad == 0 and out_layout == "TR":
        host = plan.apply_host(X, flags=hflags)
        for l in range(L + 1):
            for k in range(K):
                if not np.array_equal(host[l][k], got[l][k], equal_nan=True): fails.append("apply_host(flags %d) plane (%d, %d) differs from the device apply" % (hflags, l, k))
    plan.close()
    return tag, fails


def flags_case(i, rng, run=True):
    """FUZZ_FLAGS=1: single plans on the fallback routes of the table above lcv_pick (csrc/wagg_sparse.hip): row_len given or
    not, flags 0 / NO_LC / NO_STREAM / NO_LINES and their pairs, over compact tables with (mostly) a giant region, sometimes
    null labels, NaN / 0 weights; NaN and sometimes +-inf data, either layout of data and result, padded / unaligned rows; the
    plain aggregation and one of: nothing more, one power, fused powers K = 1..5, 1..6 degree-day thresholds.  Every plane
    against the oracle, the second plain apply bit for bit the first.  The tag names the route by that table -- [route A]: no
    whole-line chunking, flags otherwise 0; [route C]: NO_LC; [route D]: NO_STREAM; [route F]: the default -- and [edd on
    gather] where degree days run on a plan without the loader/consumer kernel.  run=False: the tag alone, from the same
    random stream (no GPU)."""
    from climate_toolbox_amd import _lib
    dtype = np.float32 if rng.random() < 0.5 else np.float64
    rtol = 1e-4 if dtype == np.float32 else 1e-6
    T = int(rng.choice([1, 2, 3, 7, 16, 63, 64, 65, 100, 129, 130]))
    sc = int(os.environ.get("FUZZ_SCALE", "1"))
    nlat = int(rng.integers(4, 60 * sc))
    nlon = 4 * int(rng.integers(2, 23 * sc)) if rng.random() < 0.7 else int(rng.integers(5, 90 * sc))
    G = nlat * nlon
    bh, bw = int(rng.integers(1, 9)), int(rng.integers(1, 17))
    keep = np.flatnonzero(rng.random(G) < rng.uniform(0.3, 1.0))
    if not len(keep):
        keep = np.array([int(rng.integers(0, G))])
    nbw = (nlon + bw - 1) // bw
    reg = ((keep // nlon) // bh) * nbw + (keep % nlon) // bw
    R = int(reg.max()) + 1 + int(rng.integers(0, 3))                                   # (sometimes a region nobody maps to)
    extra = rng.choice(keep, min(len(keep), 40))
    cell = np.concatenate([keep, extra]).astype(np.int32)
    code = np.concatenate([reg, rng.integers(0, R, len(extra))]).astype(np.int32)
    if rng.random() < 0.4:
        code[rng.integers(0, len(code), 3)] = -1
    giant = rng.random() < 0.6 and G > 400
    if giant:                                                                         # a run of cells plus scattered ones, as a region of its own
        n = int(rng.integers(260, min(G, 1500)))
        start = int(rng.integers(0, G - n // 2))
        cell = np.concatenate([cell, np.arange(start, start + n // 2), rng.choice(G, n - n // 2, replace=False)]).astype(np.int32)
        code = np.concatenate([code, np.full(n, R)]).astype(np.int32)
        R += 1
    w = rng.uniform(0.05, 3.0, len(cell))
    w[rng.random(len(cell)) < 0.05] = np.nan
    w[rng.random(len(cell)) < 0.03] = 0.0
    X = (288.0 + 9.0 * rng.standard_normal((T, G))).astype(dtype)
    if rng.random() < 0.6:
        X[rng.integers(0, T, 5), cell[rng.integers(0, len(cell), 5)]] = np.nan
    if rng.random() < 0.4:
        X[rng.integers(0, T), cell[rng.integers(0, len(cell))]] = np.inf
    if rng.random() < 0.3:
        X[rng.integers(0, T), cell[rng.integers(0, len(cell))]] = -np.inf
    layout = "TG" if rng.random() < 0.6 else "GT"
    out_layout = "TR" if rng.random() < 0.6 else "RT"
    pad = int(rng.choice([0, 0, 1, 3, 4]))
    row_len = nlon if rng.random() < 0.5 else 0
    LC, ST, LN = _lib.PLAN_NO_LC, _lib.PLAN_NO_STREAM, _lib.PLAN_NO_LINES
    flags = int(rng.choice([0, 0, LC, ST, LN, LC | ST, LC | LN, ST | LN]))
    kind = ["none", "power", "fused", "edd"][int(rng.choice(4, p=[0.2, 0.15, 0.25, 0.4]))]
    n = int(rng.integers(1, 5)) if kind == "power" else int(rng.integers(1, 6)) if kind == "fused" else int(rng.integers(1, 7))
    half = rng.uniform(0, 8, X.shape).astype(dtype)
    thr = [float(e) for e in rng.uniform(5, 35, 6)[:n]]
    route = "D" if flags & ST else "C" if flags & LC else "A" if (row_len == 0 or flags & LN) else "F"
    tag = "flags case %d: %s T=%d grid=%dx%d R=%d nseg=%d row_len=%d flags=%d %s->%s pad=%d %s(%d)%s [route %s]%s" % (
        i, dtype.__name__, T, nlat, nlon, R, len(cell), row_len, flags, layout, out_layout, pad, kind, n, " giant" if giant else "",
        route, " [edd on gather]" if kind == "edd" and route != "F" else "")
    if not run:
        return tag, None

    def dev(a):                                                                       # NaN in the pad; pad 1, 3: rows not 16-byte aligned
        a = torch.from_numpy(np.ascontiguousarray(a if layout == "TG" else a.T)).cuda()
        if not pad:
            return a
        buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=a.dtype, device="cuda")
        c0 = 1 if pad in (1, 3) else 0
        buf[:, c0:c0 + a.shape[1]] = a
        return buf[:, c0:c0 + a.shape[1]]

    def tr(a):
        return a if out_layout == "TR" else np.swapaxes(a, -1, -2)
    fails = []
    plan = SparsePlan(cell, code, w, G, R, row_len=row_len, flags=flags)
    Xd = dev(X)
    got = plan.apply(Xd, layout=layout, out_layout=out_layout).cpu().numpy()
    b = rel_bad(tr(got), O.agg_coded(X, cell, code, w, R), rtol, 1.0)
    if b: fails.append("apply: " + b)
    if not np.array_equal(plan.apply(Xd, layout=layout, out_layout=out_layout).cpu().numpy(), got, equal_nan=True): fails.append("the second apply differs")
    if kind in ("power", "fused"):
        p0, K = (n, 1) if kind == "power" else (1, n)
        gp = tr(plan.apply_poly(Xd, -273.15, K, layout=layout, out_layout=out_layout, pow_first=p0).cpu().numpy())
        for k in range(K):
            b = rel_bad(gp[k], O.agg_coded(O.tas_poly_values(X, p0 + k), cell, code, w, R), rtol, 10.0 ** (p0 + k))
            if b: fails.append("poly p=%d: %s" % (p0 + k, b))
    elif kind == "edd":
        lo, hi = X - half, X + half
        thr = edge_thresholds(thr, lo, hi, cell, -273.15, dtype)
        ge = tr(plan.apply_edd(dev(lo), dev(hi), thr, offset=-273.15, layout=layout, out_layout=out_layout).cpu().numpy())
        for k, e in enumerate(thr):
            b = rel_bad(ge[k], O.agg_coded(O.snyder_edd_values(lo + dtype(-273.15), hi + dtype(-273.15), e), cell, code, w, R), rtol, 0.05)
            if b: fails.append("edd e=%.2f: %s" % (e, b))
    plan.close()
    return tag, fails


def forms_case(i, rng, run=True):
    """FUZZ_FORMS=1: dense-family plans with a forced form (DensePlan.from_segments / from_csr, form="full" / "tiles" /
    "entries"; the fp32 full form split or exact) over scattered tables with duplicate rows, negative weights, sometimes null
    labels and NaN weights; zero-mean fields 10^u N(0, 1), u uniform in [-2, 2] per row, contiguous, one element into a wider
    buffer or with a padded pitch; NaN or +-inf data.  Against the oracle within rtol sum |x| |w| / |den| per (t, r) (what
    the rounding of a sum is proportional to; the split form: 4e-6 of it plus its 2^-36 floors), the second apply bit for bit
    the first; with +-inf the MFMA forms are compared in the rows without it and must raise the note once.  A pair with a
    negative weight is never repeated: the oracle multiplies row by row, a plan adds the rows of a pair first (S5), and +-inf
    data times weights of both signs of one pair is NaN in the one and +-inf in the other.  The tag names the form -- [form full] / [form tiles] / [form entries].  run=False: the tag alone, from the same random stream."""
    dtype = np.float32 if rng.random() < 0.5 else np.float64
    rtol = 1e-4 if dtype == np.float32 else 1e-6
    form = ["full", "tiles", "entries"][int(rng.integers(0, 3))]
    exact = bool(rng.random() < 0.5)
    T = int(rng.choice([1, 2, 16, 17, 63, 64, 65, 97, 127, 128, 129, 257, 369]))
    G = int(rng.choice([1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 384, 385, 640, 1000]))
    R = int(rng.choice([1, 2, 15, 16, 17, 47, 48, 49, 255, 256, 257, 688, 689, 700]))
    fill = float(rng.choice([0.02, 0.1, 0.4]))
    m = rng.random((G, R)) < fill
    if G > 64 and rng.random() < 0.7:
        m[32:64] = False                                                             # empty tiles for the tile-sparse form
    m[int(rng.integers(0, G)), int(rng.integers(0, R))] = True
    cell, code = (a.astype(np.int32) for a in np.nonzero(m))
    w = rng.uniform(0.1, 1.0, len(cell))
    neg = rng.random(len(cell)) < 0.02
    w[neg] *= -1.0
    dup = rng.integers(0, len(cell), len(cell) // 7)
    dup = dup[~neg[dup]]                                                             # (see above: negative weights stay single rows)
    cell, code, w = np.concatenate([cell, cell[dup]]), np.concatenate([code, code[dup]]), np.concatenate([w, rng.uniform(0.1, 1.0, len(dup))])
    perm = rng.permutation(len(cell))
    cell, code, w = cell[perm], code[perm], w[perm]
    if rng.random() < 0.5:
        code[rng.random(len(code)) < 0.02] = -1
        w[rng.random(len(w)) < 0.02] = np.nan
    X = (10.0 ** rng.uniform(-2, 2, (T, 1)) * rng.standard_normal((T, G))).astype(dtype)
    special = ["none", "nan", "inf"][int(rng.choice(3, p=[0.4, 0.35, 0.25]))]
    if special == "nan":
        X[rng.random(X.shape) < 0.01] = np.nan
        X[int(rng.integers(0, T))] = np.nan
    elif special == "inf":
        X[int(rng.integers(0, T)), int(rng.integers(0, G))] = np.inf
        X[int(rng.integers(0, T)), int(rng.integers(0, G))] = -np.inf
    view = ["contiguous", "unaligned", "pitched"][int(rng.integers(0, 3))]
    csr = bool(rng.random() < 0.3)
    variant = ("exact" if exact else "split") if form == "full" and dtype == np.float32 else ""
    tag = "forms case %d: %s T=%d G=%d R=%d nseg=%d fill=%.2f %s %s %s%s [form %s]%s" % (
        i, dtype.__name__, T, G, R, len(cell), fill, view, special, "csr" if csr else "coo", " " + variant if variant else "", form,
        " [split]" if variant == "split" else "")
    if not run:
        return tag, None
    fails = []
    if csr:
        order = np.argsort(cell, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=G))]).astype(np.int64)
        plan = DensePlan.from_csr(rowptr, code[order], w[order], G, R, dtype=dtype, form=form)
    else:
        plan = DensePlan.from_segments(cell, code, w, G, R, dtype=dtype, form=form)
    if plan.info["form"] != {"full": 0, "tiles": 1, "entries": 2}[form]:
        fails.append("form %d" % plan.info["form"])
    Xd = torch.from_numpy(X).cuda()
    if view != "contiguous":
        c0 = 1 if view == "unaligned" else 0
        wide = torch.full((T, (G + 8) // 4 * 4), float("nan"), dtype=Xd.dtype, device="cuda")
        wide[:, c0:c0 + G] = Xd
        Xd = wide[:, c0:c0 + G]
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = O.agg_coded(X, cell, code, w, R)
    keep = (code >= 0) & ~np.isnan(w)
    W = np.zeros((G, R))
    np.add.at(W, (cell[keep], code[keep]), w[keep])
    ax, aw = np.abs(np.where(np.isfinite(X), X, 0.0).astype(np.float64)), np.abs(W)
    with np.errstate(divide="ignore", invalid="ignore"):
        if variant == "split":
            tol = (4e-6 * (ax @ aw) + 2.0 ** -36 * ax.max(1, keepdims=True) * aw.sum(0)[None, :] +
                   2.0 ** -36 * aw.max(0)[None, :] * ax.sum(1, keepdims=True)) / np.abs(W.sum(0))[None, :]
        else:
            tol = rtol * (ax @ aw) / np.abs(W.sum(0))[None, :]
    got = plan.apply(Xd, exact=exact).cpu().numpy()
    if not np.array_equal(plan.apply(Xd, exact=exact).cpu().numpy(), got, equal_nan=True): fails.append("the second apply differs")
    rows = np.ones(T, dtype=bool)
    if special == "inf" and form != "entries":
        rows = np.isfinite(X).all(1)
        if not plan.saw_inf(): fails.append("+-inf was not noted")
    if plan.saw_inf(): fails.append("a note of +-inf that nothing explains")
    g, r, tl = got[rows].astype(np.float64), ref[rows], tol[rows]
    fin = np.isfinite(r)
    if not np.array_equal(np.isnan(g), np.isnan(r)): fails.append("NaN pattern differs at %d places" % (np.isnan(g) != np.isnan(r)).sum())
    elif not np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]): fails.append("inf values differ")
    elif not (np.abs(g[fin] - r[fin]) <= tl[fin] + 1e-300).all():
        fails.append("max err/tol %.3g" % (np.abs(g[fin] - r[fin]) / np.maximum(tl[fin], 1e-300)).max())
    plan.close()
    return tag, fails


def build_case(i, rng, run=True):
    """FUZZ_BUILD=1: the device plan builder (csrc/wagg_build.hip) on a random table of up to 40,000 rows with a random share
    of repeated rows (order-sensitive runs, tests/build_tables.py), of dropped rows, scattered or clustered, as COO, as CSR
    with shuffled columns or as CSR with sorted columns.  An fp64 plan of a random form is read back with the impulse probe:
    every stored weight within 2^-51 of the table-order pair sum, exact zeros, nnz, den within its fsum bound
    (tests/build_tables.py: check_readback); a second build, the other routes of the same table and the general-sort twin of
    a CSR route give the same bits.  The tag names the route -- [route coo] / [route csr] / [route csr_sorted]."""
    from tests import build_tables as B
    G = int(rng.choice([1, 127, 129, 300, 1000]))
    R = int(rng.choice([3, 37, 100, 689]))
    n_valid = int(min(rng.integers(1, 40001), 0.8 * G * (R - 1)))
    p_run = float(rng.choice([0.0, 0.1, 0.5]))
    n_drop = int(n_valid * float(rng.choice([0.0, 0.0, 0.02, 0.3])))
    order = "scattered" if rng.random() < 0.7 else "csr"
    route = ["coo", "csr", "csr_sorted"][int(rng.integers(0, 3))]
    form = ["full", "tiles", "entries"][int(rng.integers(0, 3))]
    seed = int(rng.integers(0, 2 ** 31))
    tag = "build case %d: G=%d R=%d n_valid=%d n_drop=%d p_run=%.1f %s %s [route %s]" % (i, G, R, n_valid, n_drop, p_run, order, form, route)
    if not run:
        return tag, None
    t = B.random_table("fuzz", n_valid, n_drop, G, R, seed, p_run=p_run, order=order)
    ref, cells = t.ref(), B.probe_cells(t)
    X = torch.zeros((len(cells), G), dtype=torch.float64, device="cuda")
    X[torch.arange(len(cells), device="cuda"), torch.from_numpy(cells).cuda()] = torch.from_numpy(B.amplitudes(cells)).cuda()
    field = torch.from_numpy(np.random.default_rng(seed).standard_normal((17, G))).cuda()

    def read(rt, general_sort=False):
        if rt == "coo":
            plan = DensePlan.from_segments(*t.coo(), G, R, dtype=np.float64, form=form)
        else:
            arrays = t.csr(sort_columns=rt == "csr_sorted")
            plan = DensePlan.from_csr(*arrays, G, R, dtype=np.float64, form=form, general_sort=general_sort)
            if plan.info["one_pass_sort"] != t.expect_one_pass(arrays[0], arrays[1], general_sort):
                fails.append("%s: one_pass_sort %d" % (rt, plan.info["one_pass_sort"]))
        out = (plan.info["nnz"], plan.den.copy(), plan.apply(X).cpu().numpy(), plan.apply(field).cpu().numpy())
        plan.close()
        return out

    fails = []
    first = read(route)
    try:
        B.check_readback(ref, cells, B.Readback(*first[:3]))
    except AssertionError as e:
        fails.append(str(e).splitlines()[0])
    others = [("second build", route, False)] + [(rt, rt, False) for rt in ("coo", "csr", "csr_sorted") if rt != route]
    others += [("general sort of " + rt, rt, True) for rt in ("csr", "csr_sorted")]
    for what, rt, gs in others:
        got = read(rt, gs)
        if got[0] != first[0] or not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[1:], first[1:])):
            fails.append("%s differs from %s" % (what, route))
    return tag, fails


def elements_case(i, rng, run=True):
    """FUZZ_ELEMENTS=1: one of the data-movement kernels of csrc/wagg_util.hip -- engine.relayout, to_float64, take_axis or
    gather -- on a random element type, 1 to 6 dims of extents 1 to 9, a view with random steps and starts inside a larger
    buffer (relayout, to_float64), a random order of the dims, a random axis and index list (take_axis), random cells, layouts
    and a pitched field (gather).  Random 32- / 64-bit words with NaNs, infinities, -0 and subnormals planted; results compared
    as bits with the restatements of tests/element_ops.py.  The tag names the kernel -- [kernel relayout] / [kernel to_float64]
    / [kernel take_axis] / [kernel gather].  run=False: the tag alone, from the same random stream."""
    from tests import element_ops as E
    kernel = ["relayout", "to_float64", "take_axis", "gather"][int(rng.integers(0, 4))]
    dtype = np.float32 if rng.random() < 0.5 else np.float64
    kind = E.TO_F64_KINDS[int(rng.integers(0, len(E.TO_F64_KINDS)))]
    nd = int(rng.integers(1, 7))
    shape = [int(rng.integers(1, 10)) for _ in range(nd)]
    steps = [int(rng.integers(1, 4)) for _ in range(nd)]
    starts = [int(rng.integers(0, 2)) for _ in range(nd)]
    order = [int(k) for k in rng.permutation(nd)]
    axis = int(rng.integers(-nd, nd))
    idx = rng.integers(0, shape[axis], int(rng.integers(0, 2 * shape[axis] + 2)))
    nseg = int(rng.choice([0, 1, 7, 255, 256, 257, 600]))
    layout, out_layout = ("TG" if rng.random() < 0.5 else "GT"), ("TR" if rng.random() < 0.5 else "RT")
    seed = int(rng.integers(0, 2 ** 31))
    what = {"relayout": "%s steps=%r starts=%r order=%r" % (dtype.__name__, steps, starts, order),
            "to_float64": "%s steps=%r starts=%r order=%r" % (kind, steps, starts, order),
            "take_axis": "%s axis=%d n_idx=%d" % (dtype.__name__, axis, len(idx)),
            "gather": "%s nseg=%d %s->%s pitch+%d" % (dtype.__name__, nseg, layout, out_layout, steps[0] - 1)}[kernel]
    tag = "elements case %d: shape=%r %s [kernel %s]" % (i, shape, what, kernel)
    if not run:
        return tag, None
    from climate_toolbox_amd import engine
    fails = []
    big = [b + s * st for b, s, st in zip(starts, shape, steps)]
    cut = tuple(slice(b, b + s * st, st) for b, s, st in zip(starts, shape, steps))
    n = int(np.prod(big))

    def typed(kind, values):
        if kind == "float16":
            return torch.from_numpy(values.view(np.float16).copy()).cuda()
        if kind == "bfloat16":
            return torch.from_numpy(values.view(np.int16).copy()).cuda().view(torch.bfloat16)
        return torch.from_numpy(values.copy()).cuda()

    if kernel in ("relayout", "to_float64"):
        pos = np.arange(n, dtype=np.int64)
        v = E._describe(tag, pos, pos.reshape(big)[cut], order)
        if kernel == "relayout":
            data = E.random_words(n, dtype, seed)
            got = engine.relayout(torch.as_strided(torch.from_numpy(data).cuda(), v.shape, v.strides, v.base), v.order).cpu().numpy()
            why = E.same_f64(got, E.relayout_ref(data, v), exact_nan=True)
        else:
            pool = E.to_f64_values(kind, seed % 1000)
            values = pool[np.random.default_rng(seed).integers(0, len(pool), n)]
            got = engine.to_float64(torch.as_strided(typed(kind, values), v.shape, v.strides, v.base), v.order).cpu().numpy()
            why = E.same_f64(got, E.relayout_ref(E.to_f64_ref(kind, values), v), exact_nan=kind == "float64")
        if why: fails.append("%s: %s" % (kernel, why))
    elif kernel == "take_axis":
        a = E.random_words(int(np.prod(shape)), dtype, seed).reshape(shape)
        got = engine.take_axis(torch.from_numpy(a).cuda(), axis, idx).cpu().numpy()
        why = E.same_f64(got, np.take(a, idx, axis=axis), exact_nan=True)
        if why: fails.append("take_axis: " + why)
    else:
        T, G = shape[0], int(np.prod(shape[1:]))
        X = E.random_words(T * G, dtype, seed).reshape(T, G)
        a = X if layout == "TG" else np.ascontiguousarray(X.T)
        wide = torch.full((a.shape[0], a.shape[1] + steps[0] - 1), float("nan"), dtype=torch.from_numpy(a).dtype, device="cuda")
        wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
        cells = E.gather_cells(G, nseg, seed)
        got = engine.gather(wide[:, :a.shape[1]], torch.from_numpy(cells).cuda(), layout=layout, out_layout=out_layout).cpu().numpy()
        why = E.same_f64(got, E.gather_ref(X, cells, out_layout), exact_nan=True)
        if why: fails.append("gather: " + why)
    return tag, fails


def split_case(i, rng, run=True):
    """FUZZ_SPLIT=1: the split form of an fp32 full-form plan (DensePlan.from_host; csrc/wagg_dense_split.inc) with G in
    [33, 700], R in [1, 700], T in [1, 400]: weights uniform(0.1, 1) with a random share of zeros, column r scaled by 2^j[r],
    j in [-60, 60]; rows N(0, 1) scaled by 2^k[t], k in [-100, 100], a random share of the values with a 22-bit significand
    whose f16 low part is large (tests/split_parts.py: two_part), 1 % NaN; aligned or unaligned rows.  Against the fp64
    quotient within the documented bound (4e-6 of sum |x| |w| / |den| plus the 2^-36 floors) wherever sum |x| |w| and the
    result's scale lie in [2^-110, 2^126] (a sum outside fp32's range overflows or flushes by design, as in the exact
    kernel), and against the unscaled plan bit for bit (column scales are powers of two) wherever they lie in [2^-60, 2^120]
    and the result itself is above 2^-120.  run=False: the tag alone, from the same random stream."""
    G, R, T = int(rng.integers(33, 701)), int(rng.integers(1, 701)), int(rng.integers(1, 401))
    W = rng.uniform(0.1, 1.0, (G, R)).astype(np.float32)
    W[rng.random((G, R)) < rng.uniform(0.0, 0.7)] = 0.0
    W[int(rng.integers(0, G)), :] = np.float32(0.5)                                  # (no all-zero column)
    j = rng.integers(-60, 61, R).astype(np.int32)
    k = rng.integers(-100, 101, T).astype(np.int32)
    X = rng.standard_normal((T, G))
    share = float(rng.uniform(0.0, 1.0))
    two = rng.random((T, G)) < share
    m, e = np.frexp(X)
    sig = np.sign(m) * (2 ** 21 + rng.integers(0, 1024, (T, G)) * 2 ** 11 + 513 + 2 * rng.integers(0, 512, (T, G))) * 2.0 ** -22
    X = np.ldexp(np.where(two, np.ldexp(sig, e), X).astype(np.float32), k[:, None])
    X[rng.random((T, G)) < 0.01] = np.nan
    unaligned = bool(rng.random() < 0.5)
    tag = "split case %d: T=%d G=%d R=%d two-part %.2f %s [split]" % (i, T, G, R, share, "unaligned" if unaligned else "contiguous")
    if not run:
        return tag, None
    fails = []
    Wj = np.ldexp(W, j[None, :])
    Xd = torch.from_numpy(X).cuda()
    if unaligned:
        wide = torch.full((T, (G + 8) // 4 * 4), float("nan"), dtype=Xd.dtype, device="cuda")
        wide[:, 1:1 + G] = Xd
        Xd = wide[:, 1:1 + G]
    ax, aw = np.abs(np.where(np.isnan(X), 0.0, X).astype(np.float64)), np.abs(Wj.astype(np.float64))
    den = Wj.astype(np.float64).sum(0)
    num = ax @ aw
    ref = (np.where(np.isnan(X), 0.0, X).astype(np.float64) @ Wj.astype(np.float64)) / den[None, :]
    tol = (4e-6 * num + 2.0 ** -36 * ax.max(1, keepdims=True) * aw.sum(0)[None, :] + 2.0 ** -36 * aw.max(0)[None, :] * ax.sum(1, keepdims=True)) / den[None, :]
    scale = num / den[None, :]
    ok = (num >= 2.0 ** -110) & (num <= 2.0 ** 126) & (scale >= 2.0 ** -110) & (scale <= 2.0 ** 126)
    law = (num >= 2.0 ** -60) & (num <= 2.0 ** 120) & (scale >= 2.0 ** -60) & (scale <= 2.0 ** 120) & (np.abs(ref) >= 2.0 ** -120)
    plan, base = DensePlan.from_host(Wj), DensePlan.from_host(W)
    got, plain = plan.apply(Xd).cpu().numpy(), base.apply(Xd).cpu().numpy()
    if plan.saw_inf(): fails.append("a note of +-inf that nothing explains")
    if not np.isfinite(got[ok]).all(): fails.append("non-finite results in range")
    elif not (np.abs(got[ok] - ref[ok]) <= tol[ok]).all():
        fails.append("max err/tol %.3g" % (np.abs(got[ok] - ref[ok]) / tol[ok]).max())
    if not np.array_equal(got[law], plain[law]): fails.append("the column scales change %d results" % (got[law] != plain[law]).sum())
    if ok.mean() < 0.3: fails.append("only %.2f of the results compared" % ok.mean())
    plan.close()
    base.close()
    return tag, fails


def main():
    global one_case
    if os.environ.get("FUZZ_SPLIT"):
        one_case = split_case
    if os.environ.get("FUZZ_ELEMENTS"):
        one_case = elements_case
    if os.environ.get("FUZZ_LINES"):
        one_case = lines_case
    if os.environ.get("FUZZ_MANY"):
        one_case = many_case
    if os.environ.get("FUZZ_FLAGS"):
        one_case = flags_case
    if os.environ.get("FUZZ_FORMS"):
        one_case = forms_case
    if os.environ.get("FUZZ_BUILD"):
        one_case = build_case
    rng = np.random.default_rng(SEED)
    bad = 0
    for i in range(N):
        try:
            tag, fails = one_case(i, rng)
        except Exception as e:                                                        # a crash is a failure too
            tag, fails = "case %d" % i, ["exception: %s" % traceback.format_exc().splitlines()[-1]]
        global N_LINES, N_FUSED
        N_LINES += "[lines]" in tag
        N_FUSED += "[fused]" in tag
        if fails:
            bad += 1
            print(tag, "|", "; ".join(fails), flush=True)
        if i % 25 == 24:
            print("... %d cases, %d failing" % (i + 1, bad), flush=True)
    print("fuzz: %d cases, %d failing (%d of them took the lines-only host path)" % (N, bad, N_LINES))
    if os.environ.get("FUZZ_MANY"):
        print("fuzz: %d of the many-plan cases took the fused kernel" % N_FUSED)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
