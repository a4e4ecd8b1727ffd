"""The dense-family forms at small shapes: the full form (split, exact fp32, fp64), the tile-sparse form and the entry-list
form, each forced through DensePlan.from_segments(..., form=...) and checked against host-side fp64 references.

  1  an impulse probe: T = G rows, row g holds one power of two in cell g, so out[g, r] = a_g W[g, r] / den[r] up to the
     rounding of W and den to the element type and one division -- every weight is checked on its own;
  2  zero-mean fields of very different row scales against O.agg_coded, priced by sum |x| |w| / |den| per (t, r);
  3  unaligned and pitched views, pitched results inside a sentinel border;
  4  NaN, +-inf and an overflowing transform per form (S6);
  5  the state of the pack-free passes (clean, NaN, clean data through one plan);
  6  the fused transforms per form.

Tables (host side, `table`): weights uniform(0.1, 1), a few negative, duplicate rows, null labels, NaN weights, one region
whose weights cancel to 0, and cells 32 .. 63 without a pair (so the tile-sparse form has empty tiles).  Geometry of the
entry-list form (csrc/wagg_spmm.hip: spmm_geometry): n_rb = ceil(R / 688), rw = ceil(R / (16 n_rb)), region
r = (rb 16 + wave) rw + j, chunk = cell // 128.  The 4229 x 48 table carries lists of exactly LONG_LENGTHS entries: a wave
loads 128 entries of a list at once and finishes longer ones in a one-group-at-a-time loop.

The helpers are checked without a GPU by tests/test_dense_forms_host.py."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok, torch_cuda  # noqa: F401  (torch_cuda: the parity tests' fixture)

gpu = pytest.mark.gpu

F32, F64 = np.float32, np.float64
RTOL = {F32: RTOL32, F64: RTOL64}
# the impulse probe: fl(W), fl(den) and one division, each within half an ulp: 3 u + O(u^2) < 4 u
PROBE_TOL = {F32: 2.0 ** -22, F64: 2.0 ** -51}
SPLIT_TERM = 4e-6                                                # the split form's bound per term
BK = {F32: 32, F64: 16}                                          # cells per k tile of the MFMA forms
SENTINEL = 12345.0
OFFSET = -273.15
GAP = (32, 64)                                                   # cells without a pair in every table
SMALL_TABLES = [(127, 15), (128, 16), (129, 17), (385, 688), (384, 689), (333, 257)]
LONG = (4229, 48)
LONG_WAVE = 5                                                    # the wave (regions 15 .. 17) that holds the designed lists
LONG_LENGTHS = (0, 1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 384)       # in chunks 1 .. 13 of that wave
T_ENTRY = (1, 63, 64, 65, 127, 128, 129, 257)                    # the 128- / 64-timestep blocks: ragged, full, one over
T_MFMA = T_ENTRY + (16, 17, 97, 369)
# (form, element type, variant): the fp32 full form runs split (the default) and exact
VARIANTS = [("full", F32, "split"), ("full", F32, "exact"), ("full", F64, ""), ("tiles", F32, ""), ("tiles", F64, ""),
            ("entries", F32, ""), ("entries", F64, "")]
FORM_CODE = {"full": 0, "tiles": 1, "entries": 2}


def _vid(v):
    return "-".join(x for x in (v[0], "f32" if v[1] == F32 else "f64", v[2]) if x)


# ---- host side: geometry, tables, expected values ------------------------------------------------------------------------------
def geometry(G, R):
    """(n_rb, rw, n_chunks) of the entry-list form"""
    n_rb = -(-R // 688)
    return n_rb, -(-R // (16 * n_rb)), -(-G // 128)


def coalesced(cell, code, w, R):
    """(cell, region, weight) of the distinct kept pairs: rows with a null label or a NaN weight leave, the weights of
    repeated pairs add in table order"""
    keep = (code >= 0) & ~np.isnan(w)
    key = cell[keep].astype(np.int64) * R + code[keep]
    ukey, inv = np.unique(key, return_inverse=True)
    ws = np.zeros(len(ukey))
    np.add.at(ws, inv, w[keep])
    return ukey // R, ukey % R, ws


def lists_of(cell, code, w, G, R):
    """entry counts of the coalesced table per (region block, chunk, wave)"""
    n_rb, rw, n_chunks = geometry(G, R)
    g, r, _ = coalesced(cell, code, w, R)
    counts = np.zeros((n_rb, n_chunks, 16), dtype=np.int64)
    np.add.at(counts, (r // (16 * rw), g // 128, (r // rw) % 16), 1)
    return counts


def tiles_of(cell, code, w, G, R, bk):
    """the (k tile, column tile) pairs of the MFMA forms that hold a kept pair"""
    g, r, _ = coalesced(cell, code, w, R)
    return set(zip((g // bk).tolist(), (r // 256).tolist()))


def probe_expected(cell, code, w, G, R, den=None):
    """(W, has_pair, den, W / den) of the coalesced table in fp64, W as a (G, R) matrix; `den`: the denominators to divide
    by (default: the table's own, added in table order)"""
    g, r, ws = coalesced(cell, code, w, R)
    W = np.zeros((G, R))
    has = np.zeros((G, R), dtype=bool)
    W[g, r], has[g, r] = ws, True
    if den is None:
        keep = (code >= 0) & ~np.isnan(w)
        den = np.bincount(code[keep], weights=w[keep], minlength=R)
    with np.errstate(divide="ignore", invalid="ignore"):
        return W, has, den, W / den[None, :]


def amplitudes(G):
    """a_g = +-2^k, k cycling through -3 .. 3, the sign alternating"""
    g = np.arange(G)
    return np.where(g % 2 == 0, 1.0, -1.0) * 2.0 ** (g % 7 - 3)


def probe_check(got, a, W, has, den, dtype, split=False):
    """The impulse probe's check of a (G, R) result: a pair within PROBE_TOL of a_g W / den (split form: its bound for one
    term), no pair and den != 0 an exact zero, den == 0 the IEEE result."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = a[:, None] * W / den[None, :]
        if split:
            tol = SPLIT_TERM * np.abs(a)[:, None] * np.abs(W).max(0)[None, :] / np.abs(den)[None, :]
        else:
            tol = PROBE_TOL[dtype] * np.abs(exp)
    ok = den != 0
    pair, none = has & ok[None, :], ~has & ok[None, :]
    zeros_wrong = none & (got != 0.0)
    assert not zeros_wrong.any(), "%d results without a pair are not 0, first at %s" % (zeros_wrong.sum(), np.argwhere(zeros_wrong)[0])
    with np.errstate(invalid="ignore"):
        err = np.abs(got - exp)
    bad = pair & ~(err <= tol)
    assert not bad.any(), "%d of %d weights wrong, first at (cell, region) %s: got %r, expected %r" % (
        bad.sum(), pair.sum(), np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], exp[tuple(np.argwhere(bad)[0])])
    np.testing.assert_array_equal(np.isnan(got[:, ~ok]), np.isnan(exp[:, ~ok]))
    inf = np.isinf(exp[:, ~ok])
    np.testing.assert_array_equal(got[:, ~ok][inf], exp[:, ~ok][inf])


class _Table:
    pass


def _long_pairs(rng, G, R):
    """the 4229 x 48 table: a 4 % background, and wave LONG_WAVE with lists of exactly LONG_LENGTHS entries in chunks 1 .. 13
    and of 200 .. 299 entries in chunks 14 .. 32 (its three regions hold thousands of pairs each)"""
    m = rng.random((G, R)) < 0.04
    cols = slice(3 * LONG_WAVE, 3 * LONG_WAVE + 3)
    for c in range(1, 33):
        n = LONG_LENGTHS[c - 1] if c <= len(LONG_LENGTHS) else int(rng.integers(200, 300))
        block = np.zeros(384, dtype=bool)
        block[rng.choice(384, n, replace=False)] = True
        m[128 * c:128 * (c + 1), cols] = block.reshape(128, 3)
    return m


@functools.lru_cache(maxsize=None)
def table(G, R):
    """A caller's table (cell, code, w) in random row order; see the module's docstring."""
    rng = np.random.default_rng(1000 * G + R)
    t = _Table()
    t.G, t.R = G, R
    t.r_sum0 = R // 2                                            # its weights cancel to 0: +1.5 and -1.5
    t.c_sum0 = (5, G - 2)
    m = _long_pairs(rng, G, R) if (G, R) == LONG else rng.random((G, R)) < (0.25 if R <= 32 else 0.06)
    m[GAP[0]:GAP[1], :] = False
    m[0, 0] = m[G - 1, R - 1] = True                             # the first and the last pair of the matrix
    if G > 128:
        m[128, :2] = True                                        # the first cell of the second chunk
    m[:, t.r_sum0] = False
    g, r = np.nonzero(m)
    w = rng.uniform(0.1, 1.0, len(g))
    # negative weights where a region holds several pairs (not in the cells the +-inf checks expect a positive weight in)
    big = np.flatnonzero((np.bincount(r, minlength=R)[r] >= 8) & (g != 0) & (g != 128))
    t.neg = rng.choice(big, 3, replace=False)
    w[t.neg] *= -1.0
    t.neg_pairs = [(int(g[i]), int(r[i])) for i in t.neg]
    dup = rng.integers(0, len(g), len(g) // 7)                   # repeated pairs: they add (the negative ones stay single)
    dup = dup[~np.isin(dup, t.neg)]
    g, r, w = np.concatenate([g, g[dup]]), np.concatenate([r, r[dup]]), np.concatenate([w, rng.uniform(0.1, 1.0, len(dup))])
    # null labels and NaN weights, on rows outside the designed lists and off the negative-weight pairs
    free = np.ones(len(g), dtype=bool)
    if (G, R) == LONG:
        free &= r // 3 != LONG_WAVE
    for gi, ri in t.neg_pairs + [(0, 0), (G - 1, R - 1), (128, 0), (128, 1)]:
        free &= ~((g == gi) & (r == ri))
    pick = rng.choice(np.flatnonzero(free), 2 * max(2, len(g) // 100), replace=False)
    code = r.copy()
    code[pick[:len(pick) // 2]] = -1
    w[pick[len(pick) // 2:]] = np.nan
    g = np.concatenate([g, t.c_sum0])
    code = np.concatenate([code, [t.r_sum0, t.r_sum0]])
    w = np.concatenate([w, [1.5, -1.5]])
    perm = rng.permutation(len(g))
    t.cell, t.code, t.w = g[perm].astype(np.int32), code[perm].astype(np.int32), w[perm]
    for arr in (t.cell, t.code, t.w):
        arr.setflags(write=False)
    return t


def csr_of(t):
    """the table as CSR arrays (rows = cells, the entries of a cell in table order)"""
    order = np.argsort(t.cell, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(t.cell, minlength=t.G))]).astype(np.int64)
    return rowptr, t.code[order], t.w[order]


@functools.lru_cache(maxsize=None)
def expected(G, R):
    t = table(G, R)
    out = probe_expected(t.cell, t.code, t.w, G, R)
    for arr in out:
        arr.setflags(write=False)
    return out


def den_bound(G, R):
    """what two fp64 summation orders of a region's weights can differ by: (n - 1) u sum |w|"""
    t = table(G, R)
    keep = (t.code >= 0) & ~np.isnan(t.w)
    n = np.bincount(t.code[keep], minlength=R)
    return np.maximum(n - 1, 0) * 2.0 ** -53 * np.bincount(t.code[keep], weights=np.abs(t.w[keep]), minlength=R)


@functools.lru_cache(maxsize=None)
def field(G, dtype, T, seed=0):
    """zero-mean rows of very different scales: 10^u N(0, 1), u uniform in [-2, 2] per row"""
    rng = np.random.default_rng(7919 * G + 13 * T + seed)
    X = (10.0 ** rng.uniform(-2, 2, (T, 1)) * rng.standard_normal((T, G))).astype(dtype)
    X.setflags(write=False)
    return X


def price(X, G, R, dtype, split=False):
    """The tolerance per (t, r): RTOL sum |x| |w| / |den| -- what the rounding errors of a sum are proportional to; the split
    form: its documented bound (tests/test_gpu_dense_split.py: _bound).  NaN data counts 0, +-inf rows are the caller's."""
    W, _, den, _ = expected(G, R)
    ax = np.abs(np.where(np.isfinite(X), X, 0.0).astype(np.float64))
    aw = np.abs(W)
    with np.errstate(divide="ignore", invalid="ignore"):
        if split:
            return (SPLIT_TERM * (ax @ aw) + 2.0 ** -36 * ax.max(1, keepdims=True) * aw.sum(0)[None, :] +
                    2.0 ** -36 * aw.max(0)[None, :] * ax.sum(1, keepdims=True)) / np.abs(den)[None, :]
        return RTOL[dtype] * (ax @ aw) / np.abs(den)[None, :]


def priced_ok(got, ref, tol, rows=None):
    """|got - ref| <= tol where ref is finite; NaN and +-inf as the reference has them (the rules of _rel_ok)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if rows is not None:
        got, ref, tol = got[rows], ref[rows], tol[rows]
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    err = np.abs(got[fin] - ref[fin])
    bad = ~(err <= tol[fin] + 1e-300)
    assert not bad.any(), "max err / tol %.3g at %d of %d" % ((err / np.maximum(tol[fin], 1e-300)).max(), bad.sum(), bad.size)


@functools.lru_cache(maxsize=None)
def oracle(G, R, dtype, T, seed=0):
    from oracle import ref_numpy as O
    t = table(G, R)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = O.agg_coded(field(G, dtype, T, seed), t.cell, t.code, t.w, R)
    ref.setflags(write=False)
    return ref


def _oracle_of(X, G, R):
    from oracle import ref_numpy as O
    t = table(G, R)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return O.agg_coded(X, t.cell, t.code, t.w, R)


# ---- device side ---------------------------------------------------------------------------------------------------------------
def build_plan(G, R, form, dtype, csr=False):
    from climate_toolbox_amd.engine import DensePlan
    t = table(G, R)
    if csr:
        plan = DensePlan.from_csr(*csr_of(t), G, R, dtype=dtype, form=form)
    else:
        plan = DensePlan.from_segments(t.cell, t.code, t.w, G, R, dtype=dtype, form=form)
    assert plan.info["form"] == FORM_CODE[form] and plan.dtype == np.dtype(dtype).name
    return plan


class _Ctx:
    def __init__(self, torch):
        self.torch, self._plans = torch, {}

    def plan(self, G, R, form, dtype):
        key = (G, R, form, dtype)
        if key not in self._plans:
            self._plans[key] = build_plan(G, R, form, dtype)
        return self._plans[key]

    def dev(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).cuda()

    def impulse(self, G, dtype):
        torch = self.torch
        X = torch.zeros((G, G), dtype=torch.float64 if dtype == F64 else torch.float32, device="cuda")
        i = torch.arange(G, device="cuda")
        X[i, i] = self.dev(amplitudes(G).astype(dtype))
        return X

    def close(self):
        for p in self._plans.values():
            p.close()


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    c = _Ctx(torch_cuda)
    yield c
    c.close()


def run(plan, variant, X, out=None):
    return plan.apply(X, out=out, exact=variant == "exact")


def twice(plan, variant, X):
    """the result, applied twice: the same bits (no atomics)"""
    got = run(plan, variant, X).cpu().numpy()
    np.testing.assert_array_equal(run(plan, variant, X).cpu().numpy(), got)
    return got


def check_tiles(plan, G, R, dtype):
    """the tile-sparse plan stores the tiles that hold a pair, and some hold none"""
    t = table(G, R)
    tiles = tiles_of(t.cell, t.code, t.w, G, R, BK[dtype])
    assert plan.info["n_kt"] == -(-G // BK[dtype]) and plan.info["n_nt"] == -(-R // 256)
    assert plan.info["n_tiles"] == len(tiles) < plan.info["n_kt"] * plan.info["n_nt"]


PROBE_CASES = [(G, R, v) for G, R in SMALL_TABLES for v in VARIANTS] + [(LONG[0], LONG[1], v) for v in VARIANTS if v[0] != "tiles"]
CASE_IDS = ["%dx%d-%s" % (G, R, _vid(v)) for G, R, v in PROBE_CASES]


# ---- 1. the impulse probe ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("G,R,v", PROBE_CASES, ids=CASE_IDS)
def test_impulse_probe_every_weight(ctx, G, R, v):
    """Row g of the field holds a_g = +-2^k in cell g and zeros elsewhere: out[g, r] = a_g W[g, r] / den[r].  The product is
    exact (a power of two), every other product an exact zero, so the result carries the rounding of W and of den to the
    element type and one division: 3 u < 2^-22 (fp32), 2^-51 (fp64); the split form its bound for one term.  The expected
    values divide by the plan's own fp64 denominators, which may differ from the host's sum by the order of an fp64 sum
    ((n - 1) u sum |w|, asserted) -- the apply is what the probe checks.  The same table as CSR gives the same bits."""
    form, dtype, variant = v
    t = table(G, R)
    plan = ctx.plan(G, R, form, dtype)
    counts = lists_of(t.cell, t.code, t.w, G, R)
    assert counts.shape == (geometry(G, R)[0], geometry(G, R)[2], 16)
    if (G, R) == LONG:
        assert set(LONG_LENGTHS) <= set(counts.ravel().tolist()), "the table lost a list length"
    if form == "tiles":
        check_tiles(plan, G, R, dtype)
    W, has, den, _ = expected(G, R)
    assert plan.info["nnz"] == has.sum()
    assert (np.abs(plan.den - den) <= den_bound(G, R)).all() and plan.den[t.r_sum0] == 0
    a = amplitudes(G)
    X = ctx.impulse(G, dtype)
    got = twice(plan, variant, X)
    probe_check(got, a, W, has, plan.den, dtype, split=variant == "split")
    if (G, R) != LONG:
        csr = build_plan(G, R, form, dtype, csr=True)
        try:
            np.testing.assert_array_equal(csr.den, plan.den)
            np.testing.assert_array_equal(run(csr, variant, X).cpu().numpy(), got)
        finally:
            csr.close()


# ---- 2. zero-mean fields -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("G,R,v", PROBE_CASES, ids=CASE_IDS)
def test_zero_mean_fields_priced_by_their_condition(ctx, G, R, v):
    """X = 10^u N(0, 1) with u uniform in [-2, 2] per row, against O.agg_coded in fp64 within RTOL32 / RTOL64 of
    sum |x| |w| / |den| per (t, r) (the split form: its bound); the second apply gives the same bits."""
    form, dtype, variant = v
    plan = ctx.plan(G, R, form, dtype)
    for T in (T_ENTRY if form == "entries" else T_MFMA):
        X = field(G, dtype, T)
        got = twice(plan, variant, ctx.dev(X))
        priced_ok(got, oracle(G, R, dtype, T), price(X, G, R, dtype, split=variant == "split"))


# ---- 3. views ------------------------------------------------------------------------------------------------------------------
def _aligned(v):
    return v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0


def pack_free(G, dtype, form, variant, T, aligned):
    """Does a plain apply of a clean plan start with a pack-free pass?  (csrc/wagg_dense.hip: dense_apply.)  The tile-sparse
    form: 16-byte aligned rows and G a whole number of k tiles; the full form (exact fp32, fp64) besides: two or more row
    blocks of at least 20 (fp32) / 10 (fp64) sixteen-row units."""
    if form == "entries" or variant == "split" or not aligned or G % BK[dtype]:
        return False
    if form == "tiles":
        return True
    bm_max = 16 * (23 if dtype == F32 else 11)
    n_mb = -(-T // bm_max)
    rows = -(-T // n_mb)
    mts = (1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 20, 21, 22, 23) if dtype == F32 else (1, 2, 3, 4, 5, 6, 8, 10, 11)
    mt = min(m for m in mts if 16 * m >= rows)                   # (equal row blocks: the shapes used here have no separate tail)
    return n_mb >= 2 and mt >= (20 if dtype == F32 else 10)


VIEW_CASES = [(G, R, v) for G, R in ((129, 17), (384, 689)) for v in VARIANTS]


@gpu
@pytest.mark.parametrize("G,R,v", VIEW_CASES, ids=["%dx%d-%s" % (G, R, _vid(v)) for G, R, v in VIEW_CASES])
def test_views_and_pitched_results(ctx, G, R, v):
    """The field as a view one element into a wider buffer (rows not 16-byte aligned) and as the head of rows with a padded,
    16-byte aligned pitch (the pad holds NaN), the result written into a window of a sentinel-filled buffer.  A view that
    keeps the contiguous field's route (pack-free or packed; the loads of a packing pass move bits, vector or not) gives its
    bits, one that switches the route keeps the oracle's tolerance; the border stays untouched either way."""
    torch = ctx.torch
    form, dtype, variant = v
    T = 65
    plan = ctx.plan(G, R, form, dtype)
    X = field(G, dtype, T)
    Xd = ctx.dev(X)
    ref, tol = oracle(G, R, dtype, T), price(X, G, R, dtype, split=variant == "split")
    base = run(plan, variant, Xd).cpu().numpy()
    priced_ok(base, ref, tol)
    pitch = (G + 8) // 4 * 4
    for c0 in (1, 0):
        wide = torch.full((T, pitch), float("nan"), dtype=Xd.dtype, device="cuda")
        wide[:, c0:c0 + G] = Xd
        view = wide[:, c0:c0 + G]
        assert view.stride(0) == pitch > G and _aligned(view) == (c0 == 0)
        big = torch.full((T + 2, R + 2), SENTINEL, dtype=Xd.dtype, device="cuda")
        run(plan, variant, view, out=big[1:T + 1, 1:R + 1])
        full = big.cpu().numpy()
        inner = np.zeros(full.shape, dtype=bool)
        inner[1:-1, 1:-1] = True
        assert (full[~inner] == SENTINEL).all(), "written outside the result's window"
        got = full[1:-1, 1:-1]
        priced_ok(got, ref, tol)
        if pack_free(G, dtype, form, variant, T, _aligned(view)) == pack_free(G, dtype, form, variant, T, _aligned(Xd)):
            np.testing.assert_array_equal(got, base)


# ---- 4. special values ---------------------------------------------------------------------------------------------------------
SPECIAL_CASES = [(G, R, v) for G, R in ((129, 17), (384, 689)) for v in VARIANTS]
SPECIAL_IDS = ["%dx%d-%s" % (G, R, _vid(v)) for G, R, v in SPECIAL_CASES]


def inf_sites(G, R):
    """cells for the +-inf checks: a cell with a negative weight, the first cell of the second chunk (where the padding entries
    of the entry lists point), and two cells of one region"""
    t = table(G, R)
    _, has, _, _ = expected(G, R)
    g_neg, r_neg = t.neg_pairs[0]
    r_two = int(np.flatnonzero((has.sum(0) >= 2) & (np.arange(R) != r_neg) & (np.arange(R) != t.r_sum0))[-1])
    g_two = np.flatnonzero(has[:, r_two])[:2]
    return g_neg, r_neg, 128, int(g_two[0]), int(g_two[1]), r_two


@gpu
@pytest.mark.parametrize("G,R,v", SPECIAL_CASES, ids=SPECIAL_IDS)
def test_nan_cells_count_zero(ctx, G, R, v):
    """NaN in a scattered 1 % of the cells, in a whole row and in every cell of one region (S6: the product counts 0, the
    weight stays in the denominator): the oracle's numbers, and no note of +-inf."""
    form, dtype, variant = v
    T = 65
    _, has, _, _ = expected(G, R)
    plan = ctx.plan(G, R, form, dtype)
    plan.saw_inf()
    X = np.array(field(G, dtype, T, seed=1))
    rng = np.random.default_rng(G + R)
    X[rng.random(X.shape) < 0.01] = np.nan
    X[20, :] = np.nan
    r_col = int(np.argmax(has.sum(0)))
    X[30:33, has[:, r_col]] = np.nan
    ref = _oracle_of(X, G, R)
    assert (ref[20, np.isfinite(ref[0])] == 0).all() and (ref[30:33, r_col] == 0).all()
    got = twice(plan, variant, ctx.dev(X))
    priced_ok(got, ref, price(X, G, R, dtype, split=variant == "split"))
    assert not plan.saw_inf()


@gpu
@pytest.mark.parametrize("G,R,v", SPECIAL_CASES, ids=SPECIAL_IDS)
def test_inf_per_form(ctx, G, R, v):
    """+-inf data.  The entry-list form multiplies real pairs only, so the result is the oracle's: +inf w in the regions that
    hold the cell, the sign flipped under a negative weight, NaN where +inf and -inf meet, every other region finite and
    right; its packing kernel looks for +-inf and drops what it finds (csrc/wagg_spmm.hip: spmm_pack_x_kernel writes no
    note), so saw_inf() stays false.  The MFMA forms multiply every pair of a stored tile: saw_inf() is true once, then
    false, and every row of the result without +-inf in its data matches the oracle."""
    form, dtype, variant = v
    T = 65
    _, has, _, _ = expected(G, R)
    plan = ctx.plan(G, R, form, dtype)
    plan.saw_inf()
    g_neg, r_neg, g_c1, g_a, g_b, r_two = inf_sites(G, R)
    X = np.array(field(G, dtype, T, seed=2))
    X[3, g_neg] = np.inf                                         # -inf in r_neg
    X[9, g_c1] = np.inf
    X[12, g_a] = -np.inf
    X[40, g_a], X[40, g_b] = np.inf, -np.inf                     # meet in r_two
    X[50, 0] = -np.inf
    ref = _oracle_of(X, G, R)
    assert ref[3, r_neg] == -np.inf and (ref[9, has[g_c1]] == np.inf).all() and np.isnan(ref[40, r_two])
    assert np.isfinite(ref[9, ~has[g_c1] & np.isfinite(ref[0])]).all()
    clean = np.isfinite(X).all(1)
    tol = price(X, G, R, dtype, split=variant == "split")
    got = run(plan, variant, ctx.dev(X)).cpu().numpy()
    if form == "entries":
        priced_ok(got, ref, tol)
        assert not plan.saw_inf()
    else:
        assert plan.saw_inf() and not plan.saw_inf()
        priced_ok(got, ref, tol, rows=clean)
    assert clean.sum() == T - 5


@gpu
@pytest.mark.parametrize("G,R,v", [c for c in SPECIAL_CASES if c[0] == 129], ids=[i for i in SPECIAL_IDS if i.startswith("129")])
def test_overflow_in_the_transform_sets_the_note(ctx, G, R, v):
    """(1e13 - 273.15)^3 overflows fp32 after the transform: the MFMA forms note it, fp64 and the entry-list form do not;
    the rows without the cell match the oracle."""
    from oracle import ref_numpy as O
    form, dtype, variant = v
    T = 17
    plan = ctx.plan(G, R, form, dtype)
    plan.saw_inf()
    X = (295 + 8 * np.random.default_rng(4).standard_normal((T, G))).astype(dtype)
    X[5, 70] = 1e13
    got = plan.apply_poly(ctx.dev(X), OFFSET, 3, exact=variant == "exact").cpu().numpy()
    assert plan.saw_inf() == (dtype == F32 and form != "entries")
    assert not plan.saw_inf()
    ref = _oracle_of(O.tas_poly_values(X, 3, OFFSET), G, R)
    rows = np.arange(T) != 5
    _rel_ok(got[rows], ref[rows], RTOL[dtype], scale=1e3)


# ---- 5. the state of the pack-free passes --------------------------------------------------------------------------------------
STATE_CASES = [("tiles", F32, "", 128, 16, 65), ("tiles", F64, "", 128, 16, 65), ("tiles", F32, "", 384, 689, 65),
               ("tiles", F64, "", 384, 689, 65), ("tiles", F32, "", 333, 257, 65), ("tiles", F64, "", 333, 257, 65),
               ("full", F32, "exact", 384, 689, 369), ("full", F64, "", 384, 689, 177),
               ("full", F32, "exact", 384, 689, 640), ("full", F64, "", 384, 689, 320)]


@gpu
@pytest.mark.parametrize("form,dtype,variant,G,R,T", STATE_CASES,
                         ids=["%s-%dx%d-T%d" % (_vid(c[:3]), c[3], c[4], c[5]) for c in STATE_CASES])
def test_route_state_of_the_pack_free_passes(ctx, form, dtype, variant, G, R, T):
    """One plan applies a clean field, a field with NaN and the clean field again; every result matches the oracle and, bit
    for bit, a fresh plan that sees that field alone.

    The routes (csrc/wagg_dense.hip: dense_apply): a clean plan with 16-byte aligned rows and G a whole number of k tiles
    reads X in place first; a non-finite numerator gates the packed pass on the device and leaves a sticky note, after which
    the plan packs at once.  Equal bits are what the code promises: the pack-free kernel builds by LDS-DMA the tile image the
    packing kernel writes (G % BK == 0: no padded cells; the repeated rows >= T are never read back), both run the one kernel
    body of csrc/wagg_dense_kernel.inc (the gated instantiation, DBG = 256, differs in the gate alone) over the same pieces
    and k slices, and the same reduce kernel adds the slabs in a fixed order.  So the third apply here (packed at once) and
    the fresh plan's (pack-free) compare the two routes on the same data.
    The full form takes the pack-free kernel with two or more row blocks of at least 20 (fp32) / 10 (fp64) sixteen-row
    units: T = 640 / 320 do, T = 369 / 177 (two blocks of 12 / 6 units) stay packed, like 333 x 257 (G % BK != 0)."""
    assert pack_free(G, dtype, form, variant, T, True) == ((G, T) in ((128, 65), (384, 65), (384, 640), (384, 320)))
    clean = field(G, dtype, T, seed=3)
    dirty = np.array(field(G, dtype, T, seed=4))
    dirty[T // 2, 7] = np.nan
    dirty[T - 1, G - 1] = np.nan
    one = build_plan(G, R, form, dtype)
    try:
        for X in (clean, dirty, clean):
            Xd = ctx.dev(X)
            assert _aligned(Xd) == (G % BK[dtype] == 0)
            got = run(one, variant, Xd).cpu().numpy()
            priced_ok(got, _oracle_of(X, G, R), price(X, G, R, dtype))
            fresh = build_plan(G, R, form, dtype)
            try:
                np.testing.assert_array_equal(run(fresh, variant, Xd).cpu().numpy(), got)
            finally:
                fresh.close()
        assert not one.saw_inf()
    finally:
        one.close()


# ---- 6. fused transforms -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kelvin_field(G, R, dtype, T):
    t = table(G, R)
    rng = np.random.default_rng(31 * G + T)
    X = (-OFFSET + 22 + 8 * rng.standard_normal((T, G))).astype(dtype)
    X[:, t.c_sum0[0]] = X[:, t.c_sum0[1]] + dtype(10)            # (the numerator of the region whose weights sum to 0 keeps its sign)
    X[4, 100:103] = np.nan
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def edd_fields(G, R, dtype, T):
    """(tasmin, tasmax) in degrees C, tasmin <= tasmax, NaN in one field only at a few cells"""
    t = table(G, R)
    rng = np.random.default_rng(37 * G + T)
    mean, half = 22 + 8 * rng.standard_normal((T, G)), rng.uniform(0, 8, (T, G))
    lo, hi = (mean - half).astype(dtype), (mean + half).astype(dtype)
    hi = np.maximum(lo, hi)
    lo[:, t.c_sum0[0]], hi[:, t.c_sum0[0]] = 24, 34              # (the region whose weights sum to 0: a numerator that is
    lo[:, t.c_sum0[1]], hi[:, t.c_sum0[1]] = 12, 18              #  positive or exactly 0 at every threshold)
    lo[6, 90:93] = np.nan
    hi[8, 110:113] = np.nan
    lo.setflags(write=False), hi.setflags(write=False)
    return lo, hi


EDD_THRESHOLDS = (-40.0, 22.0, 80.0)                             # below, inside and above the band of the fields


@gpu
@pytest.mark.parametrize("G,R,v", SPECIAL_CASES, ids=SPECIAL_IDS)
def test_fused_transforms_per_form(ctx, G, R, v):
    """apply_poly with powers 1 .. 4 (offset -273.15) and apply_edd with one threshold below, inside and above the band,
    against O.agg_coded of O.tas_poly_values / O.snyder_edd_values: power p relative to terms of size 10^p, degree days with
    scale 0.05 (tests/fuzz_gpu.py)."""
    from oracle import ref_numpy as O
    form, dtype, variant = v
    T = 65
    plan = ctx.plan(G, R, form, dtype)
    ex = variant == "exact"
    X = kelvin_field(G, R, dtype, T)
    Xd = ctx.dev(X)
    for p in (1, 2, 3, 4):
        got = plan.apply_poly(Xd, OFFSET, p, exact=ex).cpu().numpy()
        _rel_ok(got, _oracle_of(O.tas_poly_values(X, p, OFFSET), G, R), RTOL[dtype], scale=10.0 ** p)
    lo, hi = edd_fields(G, R, dtype, T)
    assert np.nanmin(lo) > EDD_THRESHOLDS[0] and np.nanmax(hi) < EDD_THRESHOLDS[2]
    lod, hid = ctx.dev(lo), ctx.dev(hi)
    for e in EDD_THRESHOLDS:
        got = plan.apply_edd(lod, hid, e, offset=0.0, exact=ex).cpu().numpy()
        _rel_ok(got, _oracle_of(O.snyder_edd_values(lo, hi, e), G, R), RTOL[dtype], scale=0.05)
    plan.saw_inf()


# ---- the randomised driver's forced-form cases ---------------------------------------------------------------------------------
FUZZ_FORMS_CASES, FUZZ_FORMS_SEED = 40, 2027


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


def form_counts(tags):
    return {f: sum("[form %s]" % f in tag for tag in tags) for f in ("full", "tiles", "entries")}


@gpu
def test_randomised_differential_forced_forms(ctx):
    """tests/fuzz_gpu.py's forms_case (FUZZ_FORMS=1), 40 seeded cases: forced forms, both element types, the split and the
    exact kernel, views, NaN / +-inf data, zero-mean fields priced by their condition -- every case against the oracle, each
    form at least 8 times."""
    fz = _fuzz_module()
    rng = np.random.default_rng(FUZZ_FORMS_SEED)
    failures, tags = [], []
    for i in range(FUZZ_FORMS_CASES):
        tag, fails = fz.forms_case(i, rng)
        tags.append(tag)
        assert fails is not None, "every case is compared"
        if fails:
            failures.append(tag + " | " + "; ".join(fails))
    n = form_counts(tags)
    print("forced-form cases:", n)
    assert not failures, "\n".join(failures)
    assert min(n.values()) >= 8, n
