"""The split form of the fp32 full form (csrc/wagg_dense_split.inc), part by part: what tests/split_parts.py restates and
derives, run on the device.

  1  the two-part impulse probe: T = G rows, row g holds in cell g an amplitude whose f16 low part is large, so every weight
     meets xl wh, xh wl and xh wh on its own -- within ONE_TERM (derived, 7.2e-7) of a_g W[g, r] / den[r], relative to the
     weight under test; on aligned rows, unaligned rows and a row stride that only scalar loads can follow;
  2  two cells a row, the second 2^-9 of the first: a cell scaled by a row maximum that is not its own;
  3  exponent edges of rows and columns against the fp64 quotient within the documented bound (_bound of
     tests/test_gpu_dense_split.py); exact=True beside it within RTOL32 of sum |x| |w| / |den|;
  4  scale laws bit for bit: row and column scales are powers of two and come off exactly; no state survives an apply;
  5  the fused transforms on the split path;
  6  tests/fuzz_gpu.py's split_case.

Sums whose true sum x w leaves the fp32 range overflow in the split form as they do in the exact kernel (the scales come
off before the division): by design, and not tested.  Results are normal fp32 numbers except in the rows whose largest |x|
is 2^-126 or less, where 2^-149 absolute is added (two roundings of at most 2^-150: the subnormal numerator's, kept 2^-150
by a denominator above 1, and the result's).

Plans: form "full", fp32, from DensePlan.from_segments on the tables of tests/test_gpu_dense_forms_small.py and from
DensePlan.from_host on split_parts.host_matrix (weights whose own low parts are large, small weights beside large ones)."""
import functools
import time

import numpy as np
import pytest

from tests import split_parts as S
from tests import test_gpu_dense_forms_small as D
from tests.test_gpu_dense_forms_small import PROBE_TOL, SENTINEL, SMALL_TABLES, _fuzz_module, torch_cuda  # noqa: F401
from tests.test_gpu_dense_split import _bound
from tests.test_gpu_parity import RTOL32

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = ("segments", "host")
CASES = [(G, R, k) for G, R in SMALL_TABLES for k in KINDS]
IDS = ["%dx%d-%s" % c for c in CASES]
TWO = [(129, 17), (384, 689), (333, 257)]
RATIOS = {}                                                      # the largest error / bound per case group (printed at the end)


def _note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), float(ratio))
    print("%s: largest error / bound %.3f" % (group, ratio))


@functools.lru_cache(maxsize=None)
def weights(G, R, kind):
    """(W in fp64 as the builder is given it, has_pair) of a case"""
    if kind == "segments":
        W, has, _, _ = D.expected(G, R)
        return W, has
    W = S.host_matrix(G, R).astype(np.float64)
    return W, W != 0


class _Ctx:
    def __init__(self, torch):
        self.torch, self._plans = torch, {}

    def plan(self, G, R, kind):
        from climate_toolbox_amd.engine import DensePlan
        if (G, R, kind) not in self._plans:
            p = D.build_plan(G, R, "full", F32) if kind == "segments" else DensePlan.from_host(S.host_matrix(G, R))
            assert p.info["form"] == 0 and p.dtype == "float32"
            self._plans[(G, R, kind)] = p
        return self._plans[(G, R, kind)]

    def dev(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).cuda()

    def view(self, X, way):
        """X on the device: "contiguous"; "pitched" (16-byte aligned rows, NaN in the pad: vector loads also where G % 4
        != 0); "unaligned" (one element into that buffer); "odd" (a row stride of an odd number of elements: scalar loads)"""
        torch, (T, G) = self.torch, X.shape
        Xd = self.dev(X)
        if way == "contiguous":
            return Xd
        pitch = (G + 8) // 4 * 4 + (1 if way == "odd" else 0)
        c0 = 1 if way == "unaligned" else 0
        wide = torch.full((T, pitch), float("nan"), dtype=Xd.dtype, device="cuda")
        wide[:, c0:c0 + G] = Xd
        v = wide[:, c0:c0 + G]
        assert D._aligned(v) == (way == "pitched")
        return v

    def close(self):
        for p in self._plans.values():
            p.close()


@pytest.fixture(scope="module")
def ctx(torch_cuda):  # noqa: F811
    c = _Ctx(torch_cuda)
    t0 = time.time()
    yield c
    c.close()
    print("\nsplit parts: largest error / bound per group: %s; module time %.1f s" % (
        ", ".join("%s %.3f" % kv for kv in sorted(RATIOS.items())), time.time() - t0))


def into_window(ctx, plan, Xd, R, exact=False):
    """the apply's result written into a window of a sentinel-filled, pitched tensor; the border stays untouched"""
    T = Xd.shape[0]
    big = ctx.torch.full((T + 2, R + 3), SENTINEL, dtype=Xd.dtype, device="cuda")
    plan.apply(Xd, out=big[1:T + 1, 1:R + 1], exact=exact)
    full = big.cpu().numpy()
    inner = np.zeros(full.shape, dtype=bool)
    inner[1:T + 1, 1:R + 1] = True
    assert (full[~inner] == SENTINEL).all(), "written outside the result's window"
    return full[1:T + 1, 1:R + 1]


def check_terms(got, exp, tol, pair, den, what):
    """pairs within tol of exp, exact zeros where there is no pair, the IEEE result where den == 0; returns max err / tol"""
    got = np.asarray(got, dtype=np.float64)
    ok = den != 0
    wrong = ~pair & ok[None, :] & (got != 0.0)
    assert not wrong.any(), "%s: %d results without a pair are not 0, first at %s" % (what, wrong.sum(), np.argwhere(wrong)[0])
    m = pair & ok[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(m, np.abs(got - exp) / tol, 0.0)
    bad = m & ~(ratio <= 1.0)
    assert not bad.any(), "%s: %d of %d weights wrong, largest error / bound %.3g, first at (row, region) %s: got %r, expected %r" % (
        what, bad.sum(), m.sum(), np.nanmax(ratio), np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], exp[tuple(np.argwhere(bad)[0])])
    np.testing.assert_array_equal(np.isnan(got[:, ~ok]), np.isnan(exp[:, ~ok]))
    inf = np.isinf(exp[:, ~ok])
    np.testing.assert_array_equal(got[:, ~ok][inf], exp[:, ~ok][inf])
    return ratio.max()


# ---- 1. the two-part impulse probe ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,kind", CASES, ids=IDS)
def test_two_part_impulse_probe(ctx, G, R, kind):
    """Row g holds a_g (split_parts.two_part: hi + lo == y exactly, |lo| >= 2^-13 |y|) in cell g.  Every pair lies within
    split_parts.one_term_tol of a_g W[g, r] / den[r] with the plan's own fp64 den -- ONE_TERM = 2^-21 + 2^-22 + 2^-32 of the
    term itself, derived in split_parts's docstring, plus the 2^-36 floor for the weights of floor_mask alone -- on every
    load path of the packer, bit for bit the same on all of them; exact=True meets PROBE_TOL on the same field."""
    W, has = weights(G, R, kind)
    plan = ctx.plan(G, R, kind)
    den = plan.den
    X, a = S.impulse_field(G)
    with np.errstate(invalid="ignore", divide="ignore"):
        exp = a[:, None] * W / den[None, :]
    tol = S.one_term_tol(a, W, den)
    base = None
    for way in ("contiguous", "pitched", "unaligned", "odd"):
        got = into_window(ctx, plan, ctx.view(X, way), R)
        _note("probe", check_terms(got, exp, tol, has, den, way))
        if base is None:
            base = got
        np.testing.assert_array_equal(got, base)
    ex = into_window(ctx, plan, ctx.dev(X), R, exact=True)
    with np.errstate(invalid="ignore"):
        _note("probe, exact", check_terms(ex, exp, PROBE_TOL[F32] * np.abs(exp), has, den, "exact"))
    # the restatement itself is where the device is, well inside the bound
    _note("probe against the restatement", check_terms(base, S.expected(X, W.astype(F32), den), tol, has, den, "restated"))


# ---- 2. two cells a row ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,kind", [c for c in CASES if (c[0], c[1]) in TWO], ids=[i for c, i in zip(CASES, IDS) if (c[0], c[1]) in TWO])
def test_two_cells_per_row(ctx, G, R, kind):
    """Row g holds a_g in cell g and a two-part amplitude 2^-9 times smaller in cell (g + 17) % G, whose parts are scaled by
    a_g's exponent: both still normal f16 numbers, the low one near 2^-7.  Against split_parts.expected within the sum of the
    two one-term bounds, ONE_TERM (|t1| + |t2|); where cell g has no pair in the region the small cell stands alone."""
    W, has = weights(G, R, kind)
    plan = ctx.plan(G, R, kind)
    den = plan.den
    X, a, a2, g2 = S.two_cell_field(G)
    exp = S.expected(X, W.astype(F32), den)
    with np.errstate(invalid="ignore", divide="ignore"):
        tol = S.one_term_tol(a, W, den) + S.one_term_tol(a2, W[g2], den)
    pair = has | has[g2]
    for way in ("contiguous", "unaligned"):
        got = into_window(ctx, plan, ctx.view(X, way), R)
        _note("two cells", check_terms(got, exp, tol, pair, den, way))
    alone = pair & ~has & (den != 0)[None, :]
    assert alone.sum() > 20
    with np.errstate(invalid="ignore", divide="ignore"):
        _note("two cells, the small one alone", (np.abs(got - exp) / tol)[alone].max())


# ---- 3. exponent edges -----------------------------------------------------------------------------------------------------------
def _edge_check(got, ref, tol, mask, what):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got[mask]).all(), what
    ratio = np.where(mask, np.abs(got - ref) / tol, 0.0)
    bad = np.argwhere(ratio > 1)
    assert not len(bad), "%s: %d outside the bound, largest error / bound %.3g, first at %s: got %r, expected %r" % (
        what, len(bad), ratio.max(), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
    return ratio.max()


@pytest.mark.parametrize("G,R", [(129, 17), (384, 689)])
def test_exponent_edges_of_rows(ctx, G, R):
    """split_parts.edge_rows (largest |x| of 2^-149, 2^-127, 2^-126, 2^-126 (2 - 2^-22), 1, 2^127, FLT_MAX, -FLT_MAX alone;
    zeros, NaN, -0.0; FLT_MAX beside 2^-100) through split_parts.edge_matrix: the fp64 quotient within _bound, plus 2^-149
    where the true result is below 2^-126.  exact=True: RTOL32 of sum |x| |w| / |den| plus the same 2^-149."""
    from climate_toolbox_amd.engine import DensePlan
    X, W = S.edge_rows(G), S.edge_matrix(G, R)
    den = W.astype(np.float64).sum(0)
    ref = S.true_quotient(X, W, den)
    tiny = np.where(np.abs(ref) < 2.0 ** -126, 2.0 ** -149, 0.0)
    Xz = np.where(np.isnan(X), 0.0, X).astype(np.float64)
    plan = DensePlan.from_host(W)
    try:
        np.testing.assert_array_equal(plan.den, den)
        for way in ("contiguous", "unaligned"):
            got = plan.apply(ctx.view(X, way)).cpu().numpy()
            for i, name in enumerate(S.EDGE_ROW_NAMES):
                rows = np.zeros(ref.shape, dtype=bool)
                rows[i] = True
                r = _edge_check(got, ref, _bound(X, W) + tiny, rows, "row of " + name)
                print("row %-22s split error / bound %.3g" % (name, r))
                _note("edge rows", r)
            assert (got[8:11] == 0).all() and not np.isnan(got).any()
        ex = plan.apply(ctx.dev(X), exact=True).cpu().numpy()
        tol = RTOL32 * (np.abs(Xz) @ np.abs(W.astype(np.float64))) / np.abs(den)[None, :] + tiny
        _note("edge rows, exact", _edge_check(ex, ref, tol, np.ones(ref.shape, dtype=bool), "exact"))
        assert not plan.saw_inf()
    finally:
        plan.close()


@pytest.mark.parametrize("G,R", [(129, 17), (384, 689)])
def test_exponent_edges_of_columns(ctx, G, R):
    """split_parts.edge_columns: column maxima of 2^-140 (subnormal weights, a subnormal fp32 denominator), 2^-126 and 2^100,
    and an all-zero column (NaN), under rows of 2^120 .. 2^-118: every (row, column) whose products, numerator and result are
    normal numbers (edge_valid) against the fp64 quotient within _bound plus what rounding den to fp32 can move it by
    (den_format_term: 2^-24 of the result, more in the column whose denominator is subnormal)."""
    from climate_toolbox_amd.engine import DensePlan
    W, X = S.edge_columns(G, R)
    den = W.astype(np.float64).sum(0)
    ok = S.edge_valid(X, W)
    ref = S.true_quotient(X, W, den)
    plan = DensePlan.from_host(W)
    try:
        np.testing.assert_array_equal(plan.den, den)
        with np.errstate(invalid="ignore", divide="ignore"):
            tol = _bound(X, W) + S.den_format_term(ref, den)
        got = plan.apply(ctx.dev(X)).cpu().numpy()
        assert np.isnan(got[:, S.EDGE_COL_ZERO]).all()
        for c in (0, 1, 2):
            m = np.zeros(ok.shape, dtype=bool)
            m[:, c] = ok[:, c]
            r = _edge_check(got, ref, tol, m, "column %d" % c)
            print("column of 2^%d: %d rows, split error / bound %.3g" % (np.log2(S.EDGE_COLS[c]), m.sum(), r))
        _note("edge columns", _edge_check(got, ref, tol, ok, "all columns"))
        ex = plan.apply(ctx.dev(X), exact=True).cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            tol = RTOL32 * np.abs(ref) + S.den_format_term(ref, den)       # (all values >= 0: sum |x| |w| / |den| is the result)
        _note("edge columns, exact", _edge_check(ex, ref, tol, ok, "exact"))
    finally:
        plan.close()


# ---- 4. scale laws, bit for bit --------------------------------------------------------------------------------------------------
LAW_TABLES = [(333, 257), (384, 689)]


@functools.lru_cache(maxsize=None)
def law_field(G, T):
    rng = np.random.default_rng(G + T)
    X = (280 + 30 * rng.standard_normal((T, G))).astype(F32)
    X.setflags(write=False)
    return X


def _host_w(G, R):
    W, _, _, _ = D.expected(G, R)
    return W.astype(F32)


@pytest.mark.parametrize("G,R", LAW_TABLES)
def test_row_and_column_scales_come_off_exactly(ctx, G, R):
    """diag(2^k) X with k in [-100, 100] per row scales row t of the result by 2^k[t]; W diag(2^j) with j in [-60, 60] per
    column leaves the result as it is and scales den; reversed and permuted rows (T = 400: two row blocks) give the permuted
    rows.  Every one bit for bit."""
    from climate_toolbox_amd.engine import DensePlan
    rng = np.random.default_rng(G * R)
    T = 97
    X = law_field(G, T)
    seg = ctx.plan(G, R, "segments")
    W = _host_w(G, R)
    for plan in (seg, None):
        plan = plan or DensePlan.from_host(W)
        out = plan.apply(ctx.dev(X)).cpu().numpy()
        k = rng.integers(-100, 101, T)
        Xk = np.ldexp(X, k[:, None].astype(np.int32))
        assert np.isfinite(Xk).all() and (np.ldexp(Xk, -k[:, None].astype(np.int32)) == X).all()
        with np.errstate(invalid="ignore"):
            np.testing.assert_array_equal(plan.apply(ctx.dev(Xk)).cpu().numpy(), np.ldexp(out, k[:, None].astype(np.int32)))
        np.testing.assert_array_equal(plan.apply(ctx.dev(X[::-1])).cpu().numpy(), out[::-1])
        X4 = law_field(G, 400)
        out4 = plan.apply(ctx.dev(X4)).cpu().numpy()
        perm = rng.permutation(400)
        assert (perm[:200] >= 200).any()
        np.testing.assert_array_equal(plan.apply(ctx.dev(X4[perm])).cpu().numpy(), out4[perm])
        np.testing.assert_array_equal(plan.apply_host(np.array(X)), out)
        if plan is not seg:
            j = rng.integers(-60, 61, R)
            Wj = np.ldexp(W, j[None, :].astype(np.int32))
            scaled = DensePlan.from_host(Wj)
            try:
                np.testing.assert_array_equal(scaled.den, np.ldexp(plan.den, j.astype(np.int32)))
                np.testing.assert_array_equal(scaled.apply(ctx.dev(X)).cpu().numpy(), out)
            finally:
                scaled.close()
                plan.close()


@pytest.mark.parametrize("G,R", LAW_TABLES)
def test_no_state_survives_an_apply(ctx, G, R):
    """After an apply of 2^20 X, of an all-NaN field and of a field with one +inf, an apply of X gives the bits of a fresh
    plan's first apply (the row maxima are taken anew); +inf sets the note once and the clean apply leaves it clear."""
    T = 97
    X = law_field(G, T)
    fresh = D.build_plan(G, R, "full", F32)
    one = D.build_plan(G, R, "full", F32)
    try:
        first = fresh.apply(ctx.dev(X)).cpu().numpy()
        assert not fresh.saw_inf()
        Xi = np.array(X)
        Xi[40, 0] = np.inf
        for other, inf in ((np.ldexp(X, 20), False), (np.full_like(X, np.nan), False), (Xi, True)):
            got = one.apply(ctx.dev(other)).cpu().numpy()
            assert one.saw_inf() == inf and not one.saw_inf()
            if inf:
                clean = np.arange(T) != 40
                np.testing.assert_array_equal(got[clean], first[clean])
            np.testing.assert_array_equal(one.apply(ctx.dev(X)).cpu().numpy(), first)
            assert not one.saw_inf()
    finally:
        fresh.close()
        one.close()


# ---- 5. transforms on the split path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,kind", [(129, 17, "segments"), (384, 689, "host")])
def test_transforms_on_the_split_path(ctx, G, R, kind):
    """apply_poly (offset -273.15, powers 1 .. 4) and apply_edd on the two-part impulse field.  The library's own element
    transform (engine.transform_poly / transform_edd: pinned bit for bit by test_gpu_element_ops and test_gpu_edd_edges) of
    the field, pushed through split_parts.expected, is the expected value.  The transformed field has no zero cell, so a
    result is a sum of G terms whose fp32 additions the restatement does not have: within the documented bound (_bound)."""
    from climate_toolbox_amd import engine
    W, has = weights(G, R, kind)
    W32 = W.astype(F32)
    plan = ctx.plan(G, R, kind)
    den = plan.den
    ok = np.broadcast_to((den != 0)[None, :], (G, R))
    X, _ = S.impulse_field(G)
    X = X + F32(273.15)
    Xd = ctx.dev(X)
    for p in (1, 2, 3, 4):
        Y = engine.transform_poly(Xd, D.OFFSET, p).cpu().numpy().reshape(X.shape)
        got = plan.apply_poly(Xd, D.OFFSET, p).cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            _note("transforms", _edge_check(got, S.expected(Y, W32, den), _bound(Y, W32), ok, "power %d" % p))
    lo, hi = ctx.dev(X - F32(273.15)), ctx.dev(X - F32(273.15) + F32(6))
    Y = engine.transform_edd(lo, hi, 0.0, [(1.0, 2.0)]).cpu().numpy().reshape(X.shape)
    assert (Y > 0).any()
    got = plan.apply_edd(lo, hi, 2.0).cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        _note("transforms", _edge_check(got, S.expected(Y, W32, den), _bound(Y, W32), ok, "edd"))
    # one cell whose 4th power overflows: the note is set, the other rows keep the bound
    assert not plan.saw_inf()
    Xo = np.array(X)
    Xo[3, 70] = 1e13
    Y = engine.transform_poly(ctx.dev(Xo), D.OFFSET, 4).cpu().numpy().reshape(X.shape)
    assert np.isinf(Y[3, 70]) and np.isfinite(np.delete(Y, 3, 0)).all()
    got = plan.apply_poly(ctx.dev(Xo), D.OFFSET, 4).cpu().numpy()
    assert plan.saw_inf() and not plan.saw_inf()
    rows = np.array(ok)
    rows[3] = False
    Yf = np.where(np.isinf(Y), 0.0, Y)
    with np.errstate(invalid="ignore", divide="ignore"):
        _edge_check(got, S.expected(Yf, W32, den), _bound(Yf, W32), rows, "the rows beside the overflow")


# ---- 6. the randomised driver ----------------------------------------------------------------------------------------------------
FUZZ_SPLIT_CASES, FUZZ_SPLIT_SEED = 24, 2029


def test_randomised_split_cases(ctx):
    """tests/fuzz_gpu.py's split_case (FUZZ_SPLIT=1), 24 seeded cases: per-column and per-row power-of-two scales, two-part
    values, NaN cells, aligned or unaligned rows -- the fp64 quotient within _bound, the column-scale law bit for bit."""
    fz = _fuzz_module()
    rng = np.random.default_rng(FUZZ_SPLIT_SEED)
    failures = []
    for i in range(FUZZ_SPLIT_CASES):
        tag, fails = fz.split_case(i, rng)
        assert fails is not None, "every case is compared"
        if fails:
            failures.append(tag + " | " + "; ".join(fails))
    assert not failures, "\n".join(failures)
