"""The single-plan fallback routes of the segment-table form at small shapes: sparse_stream_kernel, the non-giant arms of
sparse_gather_kernel (degree days with NTHR = 1 / 4 and several passes, (gridcell, time) data), sparse_lcv_kernel on
region-shaped chunks, the giant arm beside each of them, and fill_empty_kernel on every plane -- each against the fp64 oracle on
the transformed grid and against the default plan (whole-line chunkings) on the same data.

Routes (one SparsePlan each; which kernel a route sends a case to: the table above sparse_route in csrc/wagg_route.cpp, pinned
case by case by tests/golden/routes.json):
  A   flags = 0, no row_len            no whole-line chunking
  B   row_len, WAGG_PLAN_NO_LINES      as A, through the other arm of the constructor
  C   WAGG_PLAN_NO_LC                  D   WAGG_PLAN_NO_STREAM                  EC, ED   C, D with WAGG_PLAN_NO_LINES
  F   row_len, flags = 0               whole lines: the partner of the cross-check
Every table carries a giant region (a contiguous run plus scattered cells, more than 64 quads): the gather kernel's giant arm
runs beside every main kernel.

Grids: 40 x 36, 61 x 100, 96 x 192 and the ragged 37 x 27 (G % 4 == 3: the last quad holds three cells -- the clamped loads);
T in {1, 63, 64, 65, 130}: the last 64-timestep block ragged, full, one row over.  Tolerances are the project's: RTOL32 / RTOL64
against the oracle (degree days with scale 0.05, power p relative to terms of size 10^p as tests/fuzz_gpu.py has them), 3e-6 /
1e-13 between two summation orders (test_plan_flags_pin_the_kernel_form, test_sparse_random_cases)."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok, torch_cuda  # noqa: F401  (torch_cuda: the parity tests' fixture)

gpu = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
RTOL = {np.float32: RTOL32, np.float64: RTOL64}
TOL_ORDER = {np.float32: 3e-6, np.float64: 1e-13}                # another summation order, not another result
SENTINEL = 12345.0
OFFSET = -273.15
THRESHOLDS = {1: [25.0], 3: [20.0, 25.0, 30.0], 6: [20.0, 25.0, 30.0, 10.0, 27.5, 35.0]}
RAGGED = (37, 27)
CASES = [((40, 36), 130), ((61, 100), 65), ((96, 192), 64), (RAGGED, 63), (RAGGED, 1)]
# routes x shapes pairwise, not as a product: A, C, D at every shape, their variants at two
ROUTE_CASES = [(r, g, T) for r in ("A", "C", "D") for g, T in CASES] + \
              [("B", (40, 36), 130), ("B", RAGGED, 63), ("EC", (61, 100), 65), ("EC", RAGGED, 1), ("ED", (96, 192), 64), ("ED", RAGGED, 63)]
RC_IDS = ["%s-%dx%d-T%d" % (r, g[0], g[1], T) for r, g, T in ROUTE_CASES]


def _route_args(route, nlon):
    """(row_len, flags) of a route"""
    from climate_toolbox_amd import _lib
    NL = _lib.PLAN_NO_LINES
    return {"A": (0, 0), "B": (nlon, NL), "C": (nlon, _lib.PLAN_NO_LC), "D": (nlon, _lib.PLAN_NO_STREAM),
            "EC": (nlon, _lib.PLAN_NO_LC | NL), "ED": (nlon, _lib.PLAN_NO_STREAM | NL), "F": (nlon, 0)}[route]


# ---- tables, fields and references (host side, computed once and left unchanged) ---------------------------------------------
class _Table:
    pass


@functools.lru_cache(maxsize=None)
def _table(nlat, nlon):
    """Regions = 5 x 7 blocks of the grid with holes (several per chunk, several chunks per grid), rows in random order, then:
    a giant region, a sibling that owns the +-inf cells with weight 0, a region whose weights sum to 0, an emptied block
    region, a region whose rows all carry NaN weights and a trailing code nobody maps to (the last three: no kept row);
    null labels, NaN and zero weights, duplicate rows.  The last cells of the grid are referenced."""
    G = nlat * nlon
    rng = np.random.default_rng(100 * nlat + nlon)
    keep = rng.random(G) < 0.85
    keep[G - 4:] = True                                          # the last quad of the grid, ragged or not
    keep = np.flatnonzero(keep)
    nbw = (nlon + 6) // 7
    reg = ((keep // nlon) // 5) * nbw + (keep % nlon) // 7
    Rb = int(reg.max()) + 1
    t = _Table()
    t.nlat, t.nlon, t.G = nlat, nlon, G
    t.r_emptied, t.r_giant, t.r_zero, t.r_sum0, t.r_nanw, t.r_none = 1, Rb, Rb + 1, Rb + 2, Rb + 3, Rb + 4
    t.R = Rb + 5
    # special cells: each referenced by exactly one block region (not the emptied one), none in the last quad
    start = 40                                                   # (the giant region's run of 200 cells: no special cell in it)
    pick = rng.choice(keep[(reg != t.r_emptied) & (keep < G - 4) & ((keep < start) | (keep >= start + 200))], 24, replace=False)
    names = ["nan", "pinf", "ninf", "big", "a", "b"]
    t.c = {n: int(pick[i]) for i, n in enumerate(names)}
    t.c["sib"] = pick[6:12]                                      # the other cells of the zero-weight sibling
    t.c["nan_tmin"], t.c["nan_tmax"], t.c["flat"], t.c["exact"] = pick[12:15], pick[15:18], pick[18:21], pick[21:24]
    special = set(int(c) for c in pick)
    owner = dict(zip(keep.tolist(), reg.tolist()))
    t.owner = {n: owner[t.c[n]] for n in names}
    for k in range(2, G // 32):                                  # a whole 128-byte line of fp32 (two of fp64) without a special cell
        line = np.arange(32 * k, 32 * k + 32)
        if not special & set(line.tolist()) and np.isin(line, keep).any():
            break
    t.c["line"] = line
    holes = np.setdiff1d(np.arange(start + 200, G - 4), keep)    # the giant region: a run of 200 cells,
    t.c["ginf"] = int(holes[len(holes) // 2])                    # ... a cell only the giant region owns ...
    free = np.setdiff1d(np.arange(G), np.concatenate([pick, np.arange(start, start + 200), [t.c["ginf"]]]))
    giant = np.concatenate([np.arange(start, start + 200), rng.choice(free, 100, replace=False), [t.c["ginf"]]])   # ... scattered ones
    assert len(np.unique(giant >> 2)) > 64
    cell = [keep, giant, [t.c["pinf"], t.c["ninf"]], t.c["sib"], [t.c["a"], t.c["b"]], keep[:3]]
    code = [reg, np.full(len(giant), t.r_giant), [t.r_zero, t.r_zero], np.full(6, t.r_zero), [t.r_sum0, t.r_sum0], np.full(3, t.r_nanw)]
    w = [rng.uniform(0.05, 3.0, len(keep)), rng.uniform(0.1, 1.0, len(giant)), [0.0, 0.0], rng.uniform(0.5, 2.0, 6), [1.5, -1.5],
         np.full(3, np.nan)]
    cell, code, w = (np.concatenate([np.asarray(x, dtype=np.float64) for x in v]) for v in (cell, code, w))
    cell, code = cell.astype(np.int32), code.astype(np.int32)
    # NaN / zero weights, null labels and duplicates on rows that carry no special cell
    plain = np.flatnonzero(~np.isin(cell, pick) & (code < Rb))
    sel = rng.choice(plain, 60, replace=False)
    w[sel[:20]] = np.nan
    w[sel[20:40]] = 0.0
    code[sel[40:48]] = -1
    dup = sel[48:60]
    cell, code, w = np.concatenate([cell, cell[dup]]), np.concatenate([code, code[dup]]), np.concatenate([w, rng.uniform(0.05, 3.0, 12)])
    w[code == t.r_emptied] = np.nan
    perm = rng.permutation(len(cell))                            # (the row order of a table is arbitrary)
    t.cell, t.code, t.w = cell[perm], code[perm], w[perm]
    for a in (t.cell, t.code, t.w):
        a.setflags(write=False)
    return t


def _times(T):
    """timesteps of (NaN cell, NaN line, NaN row or None, +inf, -inf, inf in the giant region, 1e13)"""
    m = T - 1
    return min(7, m), min(20, m), (33 if T > 33 else None), min(9, m), min(50, m), min(11, m), min(5, m)


@functools.lru_cache(maxsize=None)
def _field(nlat, nlon, dtype, T):
    """(time, gridcell) temperatures in Kelvin with the special values of the issue in referenced cells"""
    t = _table(nlat, nlon)
    rng = np.random.default_rng(1000 + T)
    X = (OFFSET * -1 + 22 + 8 * rng.standard_normal((T, t.G))).astype(dtype)
    X[:, t.c["a"]] = X[:, t.c["b"]] + dtype(10)                  # (the numerator of the region whose weights sum to 0 keeps its sign)
    t_nan, t_line, t_row, t_p, t_n, t_g, t_b = _times(T)
    X[t_nan, t.c["nan"]] = np.nan
    X[t_line, t.c["line"]] = np.nan
    if t_row is not None:
        X[t_row, :] = np.nan
    X[t_p, t.c["pinf"]] = np.inf
    X[t_n, t.c["ninf"]] = -np.inf
    X[t_g, t.c["ginf"]] = np.inf
    X[t_b, t.c["big"]] = 1e13                                    # finite; its cube overflows fp32 only
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _edd_fields(nlat, nlon, dtype, T):
    """(tasmin, tasmax) in degrees C (offset 0, so that 20.0 and 25.0 are exact in fp32), tasmin <= tasmax everywhere"""
    t = _table(nlat, nlon)
    rng = np.random.default_rng(2000 + T)
    mean = 22 + 8 * rng.standard_normal((T, t.G))
    half = rng.uniform(0, 8, (T, t.G))
    lo, hi = (mean - half).astype(dtype), (mean + half).astype(dtype)
    hi = np.maximum(lo, hi)
    lo[:, t.c["a"]], hi[:, t.c["a"]] = 24, 34                    # (the region whose weights sum to 0: a numerator that is
    lo[:, t.c["b"]], hi[:, t.c["b"]] = 12, 18                    #  positive or exactly 0 at every threshold)
    lo[:, t.c["exact"]], hi[:, t.c["exact"]] = 20.0, 25.0        # thresholds 20 and 25 hit tasmin and tasmax exactly
    hi[:, t.c["flat"]] = lo[:, t.c["flat"]]                      # zero width
    lo[:, t.c["nan_tmax"]] = 22.0                                # NaN tasmax: NaN at the threshold 20, 0 at 25 and above
    hi[:, t.c["nan_tmax"]] = np.nan
    lo[:, t.c["nan_tmin"]] = np.nan                              # NaN tasmin: NaN, skipped
    t_row = _times(T)[2]
    if t_row is not None:
        lo[t_row, :] = np.nan
    lo.setflags(write=False), hi.setflags(write=False)
    return lo, hi


@functools.lru_cache(maxsize=None)
def _ref(nlat, nlon, dtype, T, power=0):
    """fp64 oracle of the plain aggregation (power 0) or of (X - 273.15) ** power, evaluated in the data's type"""
    from oracle import ref_numpy as O
    t, X = _table(nlat, nlon), _field(nlat, nlon, dtype, T)
    r = O.agg_coded(O.tas_poly_values(X, power, OFFSET) if power else X, t.cell, t.code, t.w, t.R)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _ref_edd(nlat, nlon, dtype, T, thr):
    from oracle import ref_numpy as O
    t = _table(nlat, nlon)
    lo, hi = _edd_fields(nlat, nlon, dtype, T)
    r = O.agg_coded(O.snyder_edd_values(lo, hi, thr), t.cell, t.code, t.w, t.R)
    r.setflags(write=False)
    return r


def _check(got, ref, dtype, scale):
    _rel_ok(got, ref, RTOL[dtype], scale=scale)


def _same_up_to_order(got, other, dtype, scale):
    _rel_ok(got, other, TOL_ORDER[dtype], scale=scale)


# ---- the references have the structure the cases are about (no GPU) ----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("grid,T", CASES, ids=["%dx%d-T%d" % (g[0], g[1], T) for g, T in CASES])
def test_oracle_outputs_have_the_intended_structure(grid, T, dtype):
    """The oracle's own outputs: +-inf in the regions that own the cells with a positive weight and finite values in the
    sibling that owns them with weight 0, inf in the giant region, the cube of 1e13 inf in fp32 only, 0 / 0 in the regions
    without a kept row, +-inf or NaN where the weights sum to 0, NaN rows counted 0, and the degree-day selections."""
    from oracle import ref_numpy as O
    t = _table(*grid)
    t_nan, t_line, t_row, t_p, t_n, t_g, t_b = _times(T)
    den = np.bincount(t.code[(t.code >= 0) & ~np.isnan(t.w)], weights=t.w[(t.code >= 0) & ~np.isnan(t.w)], minlength=t.R)
    assert den[t.r_sum0] == 0 and (den[[t.r_emptied, t.r_nanw, t.r_none]] == 0).all() and den[t.r_zero] > 0
    assert (t.code == -1).sum() >= 8 and np.isnan(t.w).sum() >= 20 and (t.w == 0).sum() >= 20
    for p in (0, 1, 2, 3, 4, 5):
        ref = _ref(*grid, dtype, T, p)
        assert ref[t_p, t.owner["pinf"]] == np.inf and ref[t_g, t.r_giant] == np.inf
        assert ref[t_n, t.owner["ninf"]] == (np.inf if p and p % 2 == 0 else -np.inf)
        assert np.isfinite(ref[:, t.r_zero]).all()               # weight 0 times inf: a NaN product, counted 0 (S6)
        assert np.isnan(ref[:, [t.r_emptied, t.r_nanw, t.r_none]]).all()
        assert not np.isfinite(ref[:, t.r_sum0]).any()
        if T > 33:
            assert np.isinf(ref[0, t.r_sum0])
            rest = np.delete(np.arange(t.R), [t.r_emptied, t.r_nanw, t.r_none, t.r_sum0])
            assert (ref[t_row, rest] == 0).all()
        assert np.isfinite(ref).sum() > ref.size // 2
        overflow = p >= 3 and dtype == np.float32
        assert np.isinf(ref[t_b, t.owner["big"]]) == overflow
    lo, hi = _edd_fields(*grid, dtype, T)
    assert (lo[~np.isnan(lo + hi)] <= hi[~np.isnan(lo + hi)]).all()
    e20, e25 = (O.snyder_edd_values(lo[0], hi[0], e) for e in (20.0, 25.0))
    assert (e20[t.c["exact"]] == 2.5).all() and (e25[t.c["exact"]] == 0).all()          # the two selections of snyder_edd1
    assert np.isnan(e20[t.c["nan_tmax"]]).all() and (e25[t.c["nan_tmax"]] == 0).all()
    assert np.isnan(e20[t.c["nan_tmin"]]).all() and np.isnan(e25[t.c["nan_tmin"]]).all()
    for e in THRESHOLDS[6]:
        ref = _ref_edd(*grid, dtype, T, e)
        assert np.isnan(ref[:, [t.r_emptied, t.r_nanw, t.r_none]]).all()
        assert not np.isfinite(ref[:, t.r_sum0]).any()
        assert np.isfinite(ref[:, :t.r_zero + 1]).sum() >= (t.r_zero - 1) * T - t.r_zero


# ---- device side: plans and device fields shared by the module ---------------------------------------------------------------
class _Ctx:
    def __init__(self, torch):
        self.torch, self._plans, self._dev = torch, {}, {}

    def plan(self, grid, route):
        from climate_toolbox_amd import engine
        if (grid, route) not in self._plans:
            t = _table(*grid)
            row_len, flags = _route_args(route, t.nlon)
            p = engine.SparsePlan(t.cell, t.code, t.w, t.G, t.R, row_len=row_len, flags=flags)
            assert p.info["n_giant"] >= 1, "every route carries a giant region"
            assert p.info["lines"] == (7 if route == "F" and t.nlon % 4 == 0 else 0)
            self._plans[(grid, route)] = p
        return self._plans[(grid, route)]

    def dev(self, key, make):
        if key not in self._dev:
            self._dev[key] = self.torch.from_numpy(np.array(make(), order="C")).cuda()
        return self._dev[key]

    def X(self, grid, dtype, T, layout="TG"):
        return self.dev(("X", grid, dtype, T, layout), lambda: _field(*grid, dtype, T) if layout == "TG" else _field(*grid, dtype, T).T)

    def edd(self, grid, dtype, T, layout="TG"):
        return tuple(self.dev(("edd", i, grid, dtype, T, layout), lambda: _edd_fields(*grid, dtype, T)[i] if layout == "TG"
                              else _edd_fields(*grid, dtype, T)[i].T) for i in (0, 1))

    def close(self):
        for p in self._plans.values():
            p.close()


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    c = _Ctx(torch_cuda)
    yield c
    c.close()



def _bordered(torch, like, T, R, out_layout, planes=None):
    """(block filled with a sentinel, the result's window inside it): a border of one row and one column around a plain
    result, of one plane before and after a stack of planes (which has to be contiguous)"""
    rows, cols = (T, R) if out_layout == "TR" else (R, T)
    if planes is None:
        big = torch.full((rows + 2, cols + 2), SENTINEL, dtype=like.dtype, device="cuda")
        return big, big[1:rows + 1, 1:cols + 1]
    big = torch.full((planes + 2, rows, cols), SENTINEL, dtype=like.dtype, device="cuda")
    return big, big[1:planes + 1]


def _border_untouched(big, planes=None):
    full = big.cpu().numpy()
    if planes is None:
        inner = np.zeros(full.shape, dtype=bool)
        inner[1:-1, 1:-1] = True
        assert (full[~inner] == SENTINEL).all(), "written outside the result's columns"
        return full[1:-1, 1:-1]
    assert (full[0] == SENTINEL).all() and (full[-1] == SENTINEL).all(), "written outside the result's planes"
    return full[1:-1]


def _tr(a, out_layout):
    return a if out_layout == "TR" else np.swapaxes(a, -1, -2)


def _apply(ctx, plan, what, args, layout, out_layout, R):
    """One apply into a sentinel-bordered block, and a second one: the same bits (no atomics), nothing outside the result.
    Returns the result as (planes, T, R) whatever the result layout."""
    torch = ctx.torch
    first = args[0]
    T = first.shape[0] if layout == "TG" else first.shape[1]
    outs = []
    for _ in range(2):
        if what == "plain":
            big, win = _bordered(torch, first, T, R, out_layout)
            plan.apply(first, layout=layout, out_layout=out_layout, out=win)
            outs.append(_tr(_border_untouched(big), out_layout)[None])
        elif what == "poly":
            p0, K = args[1], args[2]
            big, win = _bordered(torch, first, T, R, out_layout, K)
            plan.apply_poly(first, OFFSET, K, layout=layout, out_layout=out_layout, out=win, pow_first=p0)
            outs.append(_tr(_border_untouched(big, K), out_layout))
        else:
            thr = args[2]
            big, win = _bordered(torch, first, T, R, out_layout, len(thr))
            plan.apply_edd(first, args[1], thr, offset=0.0, layout=layout, out_layout=out_layout, out=win)
            outs.append(_tr(_border_untouched(big, len(thr)), out_layout))
    np.testing.assert_array_equal(outs[1], outs[0])
    assert not (outs[0] == SENTINEL).any(), "a column of the result was not written"
    return outs[0]


# ---- plain aggregation and powers on every route -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route,grid,T", ROUTE_CASES, ids=RC_IDS)
def test_plain_and_powers_on_every_route(ctx, route, grid, T, dtype):
    """No transform, one power (with the offset -273.15; the cube of 1e13 overflows fp32 after the transform) and fused
    powers K = 2, 4, 5 (five: one pass per power), (time, gridcell) and (gridcell, time) data, both result layouts: every
    plane against the oracle and against route F, (region, time) results the transposed bits, the second apply the same
    bits, nothing written outside the result, the regions without a kept row NaN in every plane."""
    t = _table(*grid)
    plan, planF = ctx.plan(grid, route), ctx.plan(grid, "F")
    p1 = 1 + (ROUTE_CASES.index((route, grid, T)) + (dtype == np.float64)) % 4
    for layout in ("TG", "GT"):
        Xd = ctx.X(grid, dtype, T, layout)
        calls = [("plain", (Xd,), [0]), ("poly", (Xd, p1, 1), [p1]), ("poly", (Xd, 3, 1), [3])]
        calls += [("poly", (Xd, 1, K), list(range(1, K + 1))) for K in ((2, 4, 5) if layout == "TG" else (2, 5))]
        for what, args, powers in calls:
            got = _apply(ctx, plan, what, args, layout, "TR", t.R)
            rt = _apply(ctx, plan, what, args, layout, "RT", t.R)
            np.testing.assert_array_equal(rt, got)
            if what == "plain":
                other = planF.apply(Xd, layout=layout).cpu().numpy()[None]
            else:
                other = planF.apply_poly(Xd, OFFSET, args[2], layout=layout, pow_first=args[1]).cpu().numpy()
            for i, p in enumerate(powers):
                scale = 10.0 ** p if p else 1.0
                _check(got[i], _ref(*grid, dtype, T, p), dtype, scale)
                _same_up_to_order(got[i], other[i], dtype, scale)
                assert np.isnan(got[i][:, [t.r_emptied, t.r_nanw, t.r_none]]).all()


# ---- degree days on every route ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route,grid,T", ROUTE_CASES, ids=RC_IDS)
def test_degree_days_on_every_route(ctx, route, grid, T, dtype):
    """Snyder degree days with 1, 3 and 6 thresholds (the NTHR = 1 and NTHR = 4 variants of the gather kernel, and a pass of
    four plus a pass of two), thresholds equal to tasmin and to tasmax of some cells, NaN in either field, zero width; growing
    degree days as the difference of two planes.  Every plane against the oracle and route F, both layouts of data and result."""
    from oracle import ref_numpy as O
    t = _table(*grid)
    plan, planF = ctx.plan(grid, route), ctx.plan(grid, "F")
    for layout in ("TG", "GT"):
        lo, hi = ctx.edd(grid, dtype, T, layout)
        for n in (1, 3, 6):
            thr = THRESHOLDS[n]
            got = _apply(ctx, plan, "edd", (lo, hi, thr), layout, "TR", t.R)
            if n != 3:
                np.testing.assert_array_equal(_apply(ctx, plan, "edd", (lo, hi, thr), layout, "RT", t.R), got)
            other = planF.apply_edd(lo, hi, thr, offset=0.0, layout=layout).cpu().numpy()
            for k, e in enumerate(thr):
                _check(got[k], _ref_edd(*grid, dtype, T, e), dtype, 0.05)
                _same_up_to_order(got[k], other[k], dtype, 0.05)
                assert np.isnan(got[k][:, [t.r_emptied, t.r_nanw, t.r_none]]).all()
            if n == 3:                                           # transformations.py:138-140: linear, so the planes' difference
                los, his = _edd_fields(*grid, dtype, T)
                gdd = O.agg_coded(O.snyder_gdd_values(los, his, 20.0, 30.0), t.cell, t.code, t.w, t.R)
                fin = np.isfinite(got[0]) & np.isfinite(got[2])
                with np.errstate(invalid="ignore"):             # (inf - inf where the weights sum to 0: masked)
                    diff = np.where(fin, got[0] - got[2], np.nan)
                _rel_ok(diff, np.where(fin, gdd, np.nan), RTOL[dtype], scale=0.05)


# ---- alignment and pitch -----------------------------------------------------------------------------------------------------
def _views(torch, X, pitch, c0):
    """the field as a view that starts c0 elements into rows of `pitch` elements, the rest of the buffer NaN"""
    wide = torch.full((X.shape[0], pitch), float("nan"), dtype=X.dtype, device="cuda")
    wide[:, c0:c0 + X.shape[1]] = X
    return wide[:, c0:c0 + X.shape[1]]


def _aligned(v):
    return v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0


ALIGN_CASES = [(r, g, T) for r in ("A", "C", "D") for g, T in (((40, 36), 65), (RAGGED, 63))]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route,grid,T", ALIGN_CASES, ids=["%s-%dx%d-T%d" % (r, g[0], g[1], T) for r, g, T in ALIGN_CASES])
def test_unaligned_base_and_padded_pitch(ctx, route, grid, T, dtype):
    """The field as a view one element into a wider buffer (rows not 16-byte aligned: the element-wise loads) and with a
    padded pitch whose pad holds NaN (vector loads; on the ragged grid the last quad of a row then reaches into the pad):
    the result of the contiguous field -- bit for bit where both have 16-byte aligned rows or both have not, within the
    tolerance between two summation orders otherwise.  Degree days also with an aligned tasmin and an unaligned tasmax."""
    torch = ctx.torch
    t = _table(*grid)
    plan = ctx.plan(grid, route)
    pitch = (t.G + 4) // 4 * 4 + 4                               # a multiple of four elements, at least five over G
    for layout in ("TG", "GT"):
        Xd = ctx.X(grid, dtype, T, layout)
        lo, hi = ctx.edd(grid, dtype, T, layout)
        n = Xd.shape[1]
        pitch_l = pitch if layout == "TG" else (T + 4) // 4 * 4 + 4
        want = {"plain": _apply(ctx, plan, "plain", (Xd,), layout, "TR", t.R), "poly": _apply(ctx, plan, "poly", (Xd, 2, 1), layout, "TR", t.R),
                "edd": _apply(ctx, plan, "edd", (lo, hi, THRESHOLDS[3]), layout, "TR", t.R)}
        _check(want["plain"][0], _ref(*grid, dtype, T), dtype, 1.0)
        for c0, c0_hi in ((1, 1), (0, 0), (0, 1)):
            v, vlo, vhi = _views(torch, Xd, pitch_l, c0), _views(torch, lo, pitch_l, c0), _views(torch, hi, pitch_l, c0_hi)
            assert v.stride(0) == pitch_l and _aligned(v) == (c0 == 0) and _aligned(vhi) == (c0_hi == 0) and v.shape[1] == n
            got = {"edd": _apply(ctx, plan, "edd", (vlo, vhi, THRESHOLDS[3]), layout, "TR", t.R)}
            if c0 == c0_hi:
                got["plain"] = _apply(ctx, plan, "plain", (v,), layout, "TR", t.R)
                got["poly"] = _apply(ctx, plan, "poly", (v, 2, 1), layout, "TR", t.R)
            for what, g in got.items():
                same_arm = _aligned(Xd) == (_aligned(v) if what != "edd" else _aligned(vlo) and _aligned(vhi))
                if same_arm:
                    np.testing.assert_array_equal(g, want[what])
                for k in range(len(g)):
                    _same_up_to_order(g[k], want[what][k], dtype, {"plain": 1.0, "poly": 100.0, "edd": 0.05}[what])
        for k, e in enumerate(THRESHOLDS[3]):
            _check(want["edd"][k], _ref_edd(*grid, dtype, T, e), dtype, 0.05)


@gpu
@pytest.mark.parametrize("route", ["A", "C", "D"])
def test_fp64_rows_that_end_in_half_a_quad(ctx, route):
    """fp64 with ldx == G and G % 4 == 2: every row is 16-byte aligned, yet the last quad of the grid holds two cells, and a
    load of four fp64 elements there would leave the row (and, in the last row, the field).  The stream and gather kernels
    take their clamped loads on such a grid.  (The field is the head of a buffer with one more row, which holds NaN.)"""
    from climate_toolbox_amd import engine
    from oracle import ref_numpy as O
    torch = ctx.torch
    nlat, nlon, T = 37, 26, 65
    G = nlat * nlon
    assert G % 4 == 2
    rng = np.random.default_rng(5)
    cell = np.concatenate([np.arange(G), rng.choice(G, 300, replace=False)]).astype(np.int32)
    code = np.concatenate([(np.arange(G) // nlon // 5) * 4 + (np.arange(G) % nlon) // 7, np.full(300, 32)]).astype(np.int32)
    w = rng.uniform(0.1, 2.0, len(cell))
    R = 33
    X = 295 + 8 * rng.standard_normal((T, G))
    half = rng.uniform(0, 8, (T, G))
    buf = torch.full((3, T + 1, G), float("nan"), dtype=torch.float64, device="cuda")
    for i, a in enumerate((X, X - 273.15 - half, X - 273.15 + half)):
        buf[i, :T] = torch.from_numpy(a).cuda()
    Xd, lo, hi = buf[0, :T], buf[1, :T], buf[2, :T]
    assert Xd.stride(0) == G and all(_aligned(v) for v in (Xd, lo, hi))
    row_len, flags = _route_args(route, nlon)
    plan = engine.SparsePlan(cell, code, w, G, R, row_len=row_len, flags=flags)
    try:
        assert plan.info["n_giant"] >= 1
        _rel_ok(plan.apply(Xd).cpu().numpy(), O.agg_coded(X, cell, code, w, R), RTOL64, scale=1.0)
        _rel_ok(plan.apply_poly(Xd, OFFSET, 1, pow_first=2).cpu().numpy()[0], O.agg_coded(O.tas_poly_values(X, 2), cell, code, w, R),
                RTOL64, scale=100.0)
        got = plan.apply_edd(lo, hi, THRESHOLDS[3]).cpu().numpy()
        for k, e in enumerate(THRESHOLDS[3]):
            _rel_ok(got[k], O.agg_coded(O.snyder_edd_values(X - 273.15 - half, X - 273.15 + half, e), cell, code, w, R), RTOL64, scale=0.05)
    finally:
        plan.close()


# ---- one region, one segment -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route", ["A", "C", "D", "F"])
def test_one_region_and_one_segment(ctx, route, dtype):
    """R = 1 (a region of one chunk, and the whole grid as one giant region) and a table of a single segment (R = 2: the
    other region has no row) on the 40 x 36 fields: plain, two fused powers and three thresholds, both layouts of the data,
    (region, time) results, against the oracle."""
    from climate_toolbox_amd import engine
    from oracle import ref_numpy as O
    grid, T = (40, 36), 65
    nlat, nlon = grid
    G = nlat * nlon
    rng = np.random.default_rng(3)
    block = (np.arange(8)[:, None] * nlon + np.arange(10, 18)[None, :]).ravel()
    tables = [(block, np.zeros(64), rng.uniform(0.1, 2, 64), 1), (np.arange(G), np.zeros(G), rng.uniform(0.1, 2, G), 1),
              (np.array([G - 1]), np.array([0]), np.array([2.0]), 2)]
    X, (los, his) = _field(*grid, dtype, T), _edd_fields(*grid, dtype, T)
    row_len, flags = _route_args(route, nlon)
    for cell, code, w, R in tables:
        cell, code = cell.astype(np.int32), code.astype(np.int32)
        plan = engine.SparsePlan(cell, code, w, G, R, row_len=row_len, flags=flags)
        try:
            assert plan.info["n_giant"] == (1 if len(cell) == G else 0)
            for layout in ("TG", "GT"):
                lo, hi = ctx.edd(grid, dtype, T, layout)
                for out_layout in ("TR", "RT"):
                    got = _apply(ctx, plan, "plain", (ctx.X(grid, dtype, T, layout),), layout, out_layout, R)
                    _check(got[0], O.agg_coded(X, cell, code, w, R), dtype, 1.0)
                    got = _apply(ctx, plan, "poly", (ctx.X(grid, dtype, T, layout), 1, 2), layout, out_layout, R)
                    for p in (1, 2):
                        _check(got[p - 1], O.agg_coded(O.tas_poly_values(X, p, OFFSET), cell, code, w, R), dtype, 10.0 ** p)
                    got = _apply(ctx, plan, "edd", (lo, hi, THRESHOLDS[3]), layout, out_layout, R)
                    for k, e in enumerate(THRESHOLDS[3]):
                        _check(got[k], O.agg_coded(O.snyder_edd_values(los, his, e), cell, code, w, R), dtype, 0.05)
                    if R == 2:
                        assert np.isnan(got[:, :, 1]).all()
        finally:
            plan.close()


# ---- the randomised driver's flag-route cases --------------------------------------------------------------------------------
FUZZ_FLAGS_CASES, FUZZ_FLAGS_SEED = 40, 2026


def _fuzz_module():
    spec = importlib.util.spec_from_file_location(
        "fuzz_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["fuzz_gpu.py"]
    try:
        spec.loader.exec_module(fz)
    finally:
        sys.argv = argv
    return fz


def _route_counts(tags):
    n = {r: sum("[route %s]" % r in tag for tag in tags) for r in "ACDF"}
    n["edd on gather"] = sum("[edd on gather]" in tag for tag in tags)
    return n


def test_flag_route_cases_cover_the_routes():
    """The 40 seeded cases, from their tags alone (no GPU): each of the routes A, C and D at least 8 times, degree days on the
    gather kernel at least 8 times."""
    fz = _fuzz_module()
    rng = np.random.default_rng(FUZZ_FLAGS_SEED)
    n = _route_counts([fz.flags_case(i, rng, run=False)[0] for i in range(FUZZ_FLAGS_CASES)])
    assert min(n["A"], n["C"], n["D"], n["edd on gather"]) >= 8, n


@gpu
def test_randomised_differential_flag_routes(ctx):
    """tests/fuzz_gpu.py's flags_case (FUZZ_FLAGS=1), 40 seeded cases: row_len given or not, every WAGG_PLAN_NO_* flag and
    their pairs, both element types, layouts and result layouts, padded and unaligned rows, no transform / one power / fused
    powers / 1 .. 6 thresholds, NaN / +-inf data, a giant region, null labels -- every plane of every case against the oracle."""
    fz = _fuzz_module()
    rng = np.random.default_rng(FUZZ_FLAGS_SEED)
    failures, tags = [], []
    for i in range(FUZZ_FLAGS_CASES):
        tag, fails = fz.flags_case(i, rng)
        tags.append(tag)
        assert fails is not None, "every case is compared"
        if fails:
            failures.append(tag + " | " + "; ".join(fails))
    n = _route_counts(tags)
    print("flag-route cases:", n)
    assert not failures, "\n".join(failures)
    assert min(n["A"], n["C"], n["D"], n["edd on gather"]) >= 8, n
