"""tests/split_parts.py checked without a GPU: the f16 parts against an independent conversion, the designed amplitudes, the
derived one-term bound on every table of tests/test_gpu_split_parts.py, and what the bound can see -- four mutations of the
restatement that the two-part probe must catch, three of which the power-of-two probe of tests/test_gpu_dense_forms_small.py
lets through."""
import numpy as np
import pytest

from tests import split_parts as S
from tests import test_gpu_dense_forms_small as D

F32 = np.float32
TABLES = D.SMALL_TABLES
MUTATIONS = ("xl0", "pair", "half", "ex1")                       # (a) .. (d)


def f16_rne(y):
    """y (fp64) rounded to the nearest f16, ties to even, by integer arithmetic on the scaled significand: the quantum of
    the binade [2^e, 2^(e + 1)) is 2^(max(e, -14) - 10); 65520 and above is inf"""
    y = np.asarray(y, dtype=np.float64)
    _, e = np.frexp(np.where(y == 0, 1.0, y))
    q = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)
    n = y / q                                                    # exact: q is a power of two
    f = np.floor(n)
    up = (n - f > 0.5) | ((n - f == 0.5) & (f % 2 == 1))
    r = (f + up) * q
    return np.where(np.abs(r) >= 65520.0, np.copysign(np.inf, y), r)


def test_parts_against_an_independent_f16_conversion():
    pat = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float64)
    fin = np.isfinite(pat)
    hi, lo = S.parts(pat, 0)
    np.testing.assert_array_equal(hi[fin], pat[fin])
    assert (lo[fin] == 0).all() and (hi[np.isnan(pat)] == 0).all() and (lo[~fin] == 0).all()
    np.testing.assert_array_equal(hi[np.isinf(pat)], pat[np.isinf(pat)])
    np.testing.assert_array_equal(f16_rne(pat[fin]), pat[fin])
    # the midpoints of neighbouring patterns go to the even one, a hair off a midpoint to the nearer one
    pos = np.sort(pat[fin & (pat >= 0)])
    mid = (pos[:-1] + pos[1:]) / 2
    for y in (mid, mid * (1 + 2.0 ** -40), mid * (1 - 2.0 ** -40), -mid):
        h, l = S.parts(y, 0)
        np.testing.assert_array_equal(h, f16_rne(y))
        np.testing.assert_array_equal(l, f16_rne(y - h))
    # fp32 values of every size, subnormal f16 results and overflow included, at exponents that move them about
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(6000) * 2.0 ** rng.integers(-40, 20, 6000)).astype(F32).astype(np.float64)
    for e in (0, -9, 14, 25):
        h, l = S.parts(v, e)
        y = np.ldexp(v, e)
        np.testing.assert_array_equal(h, f16_rne(y))
        fin = np.isfinite(h)
        np.testing.assert_array_equal(l[fin], f16_rne(y[fin] - h[fin]))
        assert (l[~fin] == 0).all()
        sub = fin & (h != 0) & (np.abs(h) < 2.0 ** -14)
        assert e != 0 or sub.sum() > 100
    assert list(S.split_exp([0.0, 1.0, 2.0 ** -149, S.FLT_MAX, 16384.0, 32767.9])) == [0, 14, 163, -113, 0, 0]


@pytest.mark.parametrize("G", sorted({g for g, _ in TABLES}))
def test_two_part_amplitudes(G):
    for shift, salt in ((0, 0), (9, 1)):
        a = S.two_part(G, shift, salt)                           # (asserts hi + lo == y and |lo| >= 2^-13 |y| for every g)
        assert a.dtype == np.float64 and len(a) == G
        m, _ = np.frexp(np.abs(a))
        sig = (m * 2.0 ** 22)
        assert (sig == np.floor(sig)).all() and (sig % 2 == 1).all(), "a 22-bit significand, its last bit set"
        np.testing.assert_array_equal(np.sign(a), np.where(np.arange(G) % 2 == 0, 1, -1))
        y = np.abs(a) * 2.0 ** (S.split_exp(np.abs(a)) )
        hi, lo = S.parts(y, 0)
        assert (hi == 2.0 ** 15).any() and (lo > 0).any() and (lo < 0).any()
    X, a, a2, g2 = S.two_cell_field(G)
    assert (np.count_nonzero(X, axis=1) == 2).all() and (S.finite_max(X, 1) == np.abs(a)).all()
    xh, xl = S.parts(X, S.split_exp(np.abs(a))[:, None])
    small = xl[np.arange(G), g2]
    assert (xh + xl == np.ldexp(X.astype(np.float64), S.split_exp(np.abs(a))[:, None].astype(np.int32))).all()
    assert (np.abs(small) >= 2.0 ** -14).all(), "the small cell's low part is a normal f16"


def _tables():
    for G, R in TABLES:
        W, has, den, _ = D.expected(G, R)
        yield "segments %dx%d" % (G, R), G, R, W, has, den
        Wh = S.host_matrix(G, R).astype(np.float64)
        yield "host %dx%d" % (G, R), G, R, Wh, Wh != 0, Wh.sum(0)


def _ratio(got, ref, tol, mask):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mask, np.abs(got - ref) / tol, 0.0)


def test_restated_split_meets_the_one_term_bound_on_every_table():
    worst = {}
    for name, G, R, W, has, den, in _tables():
        X, a = S.impulse_field(G)
        W32 = W.astype(F32)
        ok = has & (den != 0)[None, :]
        got = S.expected(X, W32, den)
        ref = S.true_quotient(X, W, den)
        tol = S.one_term_tol(a, W, den)
        r = _ratio(got, ref, tol, ok)
        n_floor = int((S.floor_mask(W32) & ok).sum())
        worst[name] = r.max()
        print("%-20s restated split / one-term bound: max %.3f over %d weights (%d with the floor)" % (name, r.max(), ok.sum(), n_floor))
        assert r.max() <= 1.0, name
        assert (got[~has & (den != 0)[None, :]] == 0).all()
        assert (n_floor == 0) == name.startswith("segments"), "the floor is for the small weights of the host matrices alone"
        t, c = np.argwhere(ok)[len(np.argwhere(ok)) // 2]
        assert abs(S.fsum_check(X, W32, den, t, c) - got[t, c]) <= 2.0 ** -50 * abs(got[t, c])
    assert max(worst.values()) > 0.05, "a bound that no weight comes near prices nothing"


def test_the_one_term_bound_sees_each_mutation():
    G, R = 128, 16
    W, has, den, _ = D.expected(G, R)
    X, a = S.impulse_field(G)
    ok = has & (den != 0)[None, :]
    ref, tol = S.true_quotient(X, W, den), S.one_term_tol(a, W, den)
    for mut in MUTATIONS:
        r = _ratio(S.expected(X, W.astype(F32), den, mutate=mut), ref, tol, ok)
        share = (r[ok] > 1).mean()
        print("mutation %-5s fails %5.1f %% of the %d weights, largest error / bound %.3g" % (mut, 100 * share, ok.sum(), r.max()))
        assert share > 0, mut
        if mut == "xl0":
            assert share >= 0.9
    # the two-cell rows: a lost low part of the SMALL cell shows where the row's large cell has no pair in the region
    X2, a, a2, g2 = S.two_cell_field(G)
    with np.errstate(invalid="ignore", divide="ignore"):
        t1 = np.abs(a)[:, None] * np.abs(W) / np.abs(den)[None, :]
        t2 = np.abs(a2)[:, None] * np.abs(W[g2]) / np.abs(den)[None, :]
        tol2 = S.ONE_TERM * (t1 + t2)
    ok2 = (has | has[g2]) & (den != 0)[None, :]
    base = S.expected(X2, W.astype(F32), den)
    Xs = X2.copy()
    hi, _ = S.parts(a2, S.split_exp(np.abs(a)))
    Xs[np.arange(G), g2] = np.ldexp(hi, -S.split_exp(np.abs(a)).astype(np.int32)).astype(F32)   # the small cell without its low part
    r = _ratio(S.expected(Xs, W.astype(F32), den), base, tol2, ok2)
    only_small = ok2 & ~has
    assert (r[only_small] > 1).mean() >= 0.9 and only_small.sum() > 20


def test_the_power_of_two_probe_passes_three_of_the_mutations():
    """The check of test_impulse_probe_every_weight (amplitudes +-2^k, the tolerance priced by the column's largest weight)
    run on the mutated restatement: xl is 0 in every row, so (a), (b) and (c) change nothing it asserts."""
    passed = {}
    for G, R in ((128, 16), (333, 257)):
        W, has, den, _ = D.expected(G, R)
        a = D.amplitudes(G)
        X = np.zeros((G, G), dtype=F32)
        X[np.arange(G), np.arange(G)] = a
        for mut in (None,) + MUTATIONS:
            got = S.expected(X, W.astype(F32), den, mutate=mut).astype(F32)
            try:
                D.probe_check(got, a, W, has, den, F32, split=True)
                passed[(G, mut)] = True
            except AssertionError:
                passed[(G, mut)] = False
        print("%dx%d: the power-of-two probe passes %s" % (G, R, {str(m): passed[(G, m)] for m in (None,) + MUTATIONS}))
        assert passed[(G, None)] and passed[(G, "xl0")] and passed[(G, "pair")] and passed[(G, "half")]
        assert not passed[(G, "ex1")]


def test_exponent_edge_builders():
    for G, R in ((129, 17), (384, 689)):
        X = S.edge_rows(G)
        assert X.dtype == F32 and X.shape == (len(S.EDGE_ROW_NAMES), G)
        W = S.edge_matrix(G, R)
        q = S.true_quotient(X, W, W.astype(np.float64).sum(0))
        assert (np.abs(np.where(np.isnan(X), 0, X).astype(np.float64) @ W.astype(np.float64)) < S.FLT_MAX * (1 - 2.0 ** -10)).all()
        assert np.isfinite(q).all() and (q[8:11] == 0).all() and (np.abs(q[0]) < 2.0 ** -126).all() and (np.abs(q[6]) > 2.0 ** 100).any()
        Wc, Xc = S.edge_columns(G, R)
        ex, ew = S.scales(Xc, Wc)
        assert [int(ew[c]) for c in (0, 1, 2, 3)] == [154, 140, -86, 0]
        ok = S.edge_valid(Xc, Wc)
        e = ex[:, None] + ew[None, :]
        ext = [(int(e[ok[:, c], c].min()), int(e[ok[:, c], c].max())) for c in (0, 1, 2, 4)]
        print("ex + ew over the valid pairs of columns 0, 1, 2, 4:", ext)
        assert all(lo <= want_lo and hi >= want_hi for (lo, hi), (want_lo, want_hi) in zip(ext, [(48, 148), (34, 146), (-80, 46), (-67, 147)]))
        assert not ok[:, S.EDGE_COL_ZERO].any() and ok[:, 4:].any(0).all()
        den = Wc.astype(np.float64).sum(0)
        assert 0 < den[0] < 2.0 ** -126 and den[1] >= 2.0 ** -126          # column 0's denominator is a subnormal fp32 number
        got, ref = S.expected(Xc, Wc, den), S.true_quotient(Xc, Wc, den)
        assert (np.abs(got - ref)[ok] <= 4e-6 * np.abs(ref)[ok]).all()
