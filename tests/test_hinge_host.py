"""Hinge and restricted-cubic-spline totals, the part that needs no GPU: the exports of wagg_hinge_* (include/wagg.h), their
bad-argument codes (all decided before any device call), the workspace rule, the argument checks of tas_hinge_aggregate and
tas_rcspline_aggregate that precede any device work, and an fp64 NumPy restatement of both statistics with the two properties
that make a restricted cubic spline one: 0 below the first knot, linear beyond the last."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_hinge_reduce_f32", "wagg_hinge_reduce_f64", "wagg_hinge_work_bytes")
EPS64 = float(np.finfo(np.float64).eps)


# ---- the restatement (fp64 throughout; tests/test_gpu_hinge.py forms d in the element type instead) -----------------------------
def hinge(x, k, power=1, side="above"):
    """max(+-(x - k), 0) ** power by multiplications; NaN gives 0"""
    d = np.asarray(x, dtype=np.float64) - np.float64(k)
    d = -d if side == "below" else d
    t = d.copy()
    for _ in range(power - 1):
        t = t * d
    with np.errstate(invalid="ignore"):
        return np.where(d > 0, t, 0.0)


def rcspline_coefficients(knots):
    """(ca, cb): term_j = h3(t_j) + ca[j] * h3(t_{K-1}) + cb[j] * h3(t_K),  j = 1 .. K - 2"""
    t = np.asarray(knots, dtype=np.float64)
    span = t[-1] - t[-2]
    return -(t[-1] - t[:-2]) / span, (t[-2] - t[:-2]) / span


def rcspline_terms(x, knots, normalize=False):
    """the K - 2 nonlinear terms of the restricted cubic spline with these knots, (K - 2,) + x.shape"""
    t = np.asarray(knots, dtype=np.float64)
    ca, cb = rcspline_coefficients(t)
    hA, hB = hinge(x, t[-2], 3), hinge(x, t[-1], 3)
    out = np.stack([(hinge(x, t[j], 3) + ca[j] * hA) + cb[j] * hB for j in range(len(t) - 2)])
    return out / (t[-1] - t[0]) ** 2 if normalize else out


def test_exports_version_and_constants():
    """The three symbols are declared, bound and exported; the binding's constants are the header's; the version is 0.11.0."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, engine, seasons, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1100
    for macro, value in (("WAGG_HINGE_MAX", 64), ("WAGG_HINGE_GROUP", 8), ("WAGG_HINGE_ABOVE", 0), ("WAGG_HINGE_BELOW", 1)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value == getattr(_lib, macro[5:]), macro
    assert callable(engine.hinge_reduce) and callable(seasons._hinge_totals)
    for name in ("tas_hinge_aggregate", "tas_rcspline_aggregate"):
        assert getattr(pkg, name) is getattr(transformations, name) and name in transformations.__all__, name


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, no device pointer dereferenced (every such pointer is a number no one may read)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)
    inf, nan = float("inf"), float("nan")

    def dbl(*v):
        return (C.c_double * len(v))(*v)

    asc = dbl(*range(66))
    two, co = dbl(30.0, 35.0), dbl(*([0.5] * 66))

    def call(fn, X=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win=p, offset=0.0, k=asc, n_knots=6, power=1, side=0,
             tk=None, ta=None, tb=None, flags=0, out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, T, n, ldx, rb, rows, P, n_rows, doy, win, offset, k, n_knots, power, side, tk, ta, tb, flags, out, ldo, pstride, status,
                  work, work_bytes, None)

    def refused(rc, text):
        msg = L.wagg_last_error()
        return rc == -1 and len(msg) > 0 and text in msg

    for fn in (L.wagg_hinge_reduce_f32, L.wagg_hinge_reduce_f64):
        for n_knots in (0, 65, -1):
            assert refused(call(fn, n_knots=n_knots), b"n_knots must be 1..64"), n_knots
        assert refused(call(fn, k=None), b"knots is NULL")
        for power in (0, 4, -1):
            assert refused(call(fn, power=power), b"power must be 1..3"), power
        for side in (2, -1):
            assert refused(call(fn, side=side), b"side must be"), side
        for bad in (nan, inf, -inf):
            assert refused(call(fn, k=dbl(0.0, bad, 2.0), n_knots=3), b"knot 1 is not finite"), bad
            assert refused(call(fn, offset=bad), b"offset must be finite"), bad
            assert refused(call(fn, tk=dbl(30.0, bad), ta=co, tb=co), b"tail knot"), bad
            assert refused(call(fn, tk=two, ta=dbl(0.5, bad, 0.5, 0.5, 0.5, 0.5), tb=co), b"tail coefficient 1"), bad
            assert refused(call(fn, tk=two, ta=co, tb=dbl(0.5, 0.5, bad, 0.5, 0.5, 0.5)), b"tail coefficient 2"), bad
        for kw in ({"tk": two}, {"ta": co}, {"tb": co}, {"tk": two, "ta": co}, {"tk": two, "tb": co}, {"ta": co, "tb": co}):
            assert refused(call(fn, **kw), b"tail_knots, tail_a and tail_b go together"), sorted(kw)
        assert refused(call(fn, doy=None), b"doy_dev and win_dev go together")
        assert refused(call(fn, win=None), b"doy_dev and win_dev go together")
        assert refused(call(fn, flags=64), b"unknown flags")
        assert refused(call(fn, flags=_lib.PERIOD_KEEP_NAN), b"unknown flags")
        # the family's own checks, in the family's order: sizes first, the layout behind the call's own arguments
        for kw in ({"P": -1}, {"n": -3}, {"T": -1}, {"n_rows": -1}):
            assert refused(call(fn, **kw), b"negative size"), kw
        assert refused(call(fn, P=-1, flags=64, n_knots=0), b"negative size")
        assert refused(call(fn, flags=64, n_knots=0), b"unknown flags")
        assert refused(call(fn, n_knots=0, power=7, ldx=7), b"n_knots")
        assert refused(call(fn, power=7, ldx=7), b"power")
        assert refused(call(fn, ldx=7), b"ldx / ldo smaller than n") and refused(call(fn, ldo=7), b"ldx / ldo smaller than n")
        assert refused(call(fn, pstride=15), b"out_pstride smaller than P * ldo")
        assert refused(call(fn, status=None), b"NULL")
        assert call(fn, rb=None) == -1 and call(fn, rows=None) == -1 and call(fn, out=None) == -1
        assert refused(call(fn, X=None), b"X_dev")
        assert call(fn, work=C.c_void_p(0x1004), work_bytes=64) == -1 and call(fn, work_bytes=-8) == -1
        # nothing to do is not an error -- with or without a season, a tail, either side, every power -- and touches no device
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
        assert call(fn, P=0, doy=None, win=None) == 0 and call(fn, P=0, n_knots=64, power=3, side=1) == 0
        assert call(fn, P=0, tk=two, ta=co, tb=co, power=3) == 0
        assert call(fn, n_knots=1, pstride=0, P=0, out=None) == 0


def test_work_bytes_are_the_bins_for_as_many_planes():
    from climate_toolbox_amd import _lib
    L = _lib.load()
    wb, bins = L.wagg_hinge_work_bytes, L.wagg_bin_days_work_bytes
    for args in ((0, 1, 10, 3), (63, 0, 10, 3), (63, 1, 0, 3), (63, 1, 10, 0), (-1, 1, 10, 3), (63, 1, 10, -2)):
        assert wb(*args) == 0, args
    some = 0
    for n in (1, 63, 256, 515, 1027, 24378, 1036800):
        for P in (1, 2, 3, 12, 70):
            for n_rows in (1, 9, 70, 80, 365, 3650):
                for planes in (1, 2, 8, 9, 17, 64):
                    assert wb(n, P, n_rows, planes) == bins(n, P, n_rows, planes + 1), (n, P, n_rows, planes)
                    some += wb(n, P, n_rows, planes) > 0
    assert some > 10 and wb(1027, 1, 80, 1) > 0 and wb(1036800, 12, 365, 41) == 0


@pytest.mark.parametrize("bad", [[], (), [1.0, 1.0], [0.0, float("nan")], [float("inf"), 0.0], None, ["a", "b"], [[1.0, 2.0]]])
def test_hinge_knots_are_validated_before_any_device_work(bad):
    """Not even the dataset is looked at (None stands in for it)."""
    from climate_toolbox_amd import tas_hinge_aggregate
    with pytest.raises(ValueError, match="thresholds|knots"):
        tas_hinge_aggregate(None, bad, "popwt", "hierid", {})


@pytest.mark.parametrize("bad", [[], [1.0], [1.0, 2.0], [1.0, 2.0, 2.0], [3.0, 2.0, 1.0], [0.0, 1.0, float("nan")], [0.0, 1.0, float("inf")],
                                 list(range(67)), None, ["a", "b", "c"], [[1.0, 2.0, 3.0]]])
def test_spline_knots_are_validated_before_any_device_work(bad):
    from climate_toolbox_amd import tas_rcspline_aggregate
    with pytest.raises(ValueError, match="knots"):
        tas_rcspline_aggregate(None, bad, "popwt", "hierid", {})


def _dataset():
    from climate_toolbox_amd import minixr
    tas = 280.0 + np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    return minixr.Dataset({"tas": (("time", "lat", "lon"), tas)},
                          coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})


def test_arguments_are_checked_before_any_device_work():
    """power outside 1..3, an unknown side, period=None, season= without period=, cells and leap_days outside their values, a
    power and a degree-day variable, a dataset without time: ValueError from both calls, with no GPU in sight."""
    from climate_toolbox_amd import minixr, tas_hinge_aggregate, tas_rcspline_aggregate
    from climate_toolbox_amd.transformations import tas_poly
    for power in (0, 4, 1.5, "2"):
        with pytest.raises(ValueError, match="power"):
            tas_hinge_aggregate(None, [10.0, 20.0], "popwt", "hierid", {}, power=power)
    for side in ("over", None, 0):
        with pytest.raises(ValueError, match="side"):
            tas_hinge_aggregate(None, [10.0, 20.0], "popwt", "hierid", {}, side=side)
    ds = _dataset()
    powered = tas_poly(ds, 2, "tas-poly-2")
    tas = ds["tas"]
    ds["edd"] = minixr.LazyArray(tas.values, tas.dims, edd=(tas.values + 5.0, 0.0, [(1.0, 10.0)]), name="edd")
    no_time = minixr.Dataset({"tas": (("lat", "lon"), np.zeros((2, 4), dtype=np.float32))},
                             coords={"lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})
    for call, knots in ((tas_hinge_aggregate, [10.0, 20.0]), (tas_rcspline_aggregate, [5.0, 15.0, 25.0, 30.0])):
        with pytest.raises(ValueError, match="needs period="):
            call(None, knots, "popwt", "hierid", {}, period=None)
        with pytest.raises(ValueError, match="season= needs period="):
            call(None, knots, "popwt", "hierid", {}, period=None, season=object())
        with pytest.raises(ValueError, match="cells must be"):
            call(None, knots, "popwt", "hierid", {}, cells="some")
        with pytest.raises(ValueError, match="leap_days"):
            call(None, knots, "popwt", "hierid", {}, leap_days="maybe")
        with pytest.raises(ValueError, match="plain"):
            call(powered, knots, "popwt", "hierid", {}, tas="tas-poly-2")
        with pytest.raises(ValueError, match="plain"):
            call(ds, knots, "popwt", "hierid", {}, tas="edd")
        with pytest.raises(ValueError, match="time"):
            call(no_time, knots, "popwt", "hierid", {})


def test_restated_hinges():
    """the restatement against hand values: both sides, every power, NaN and the knot itself give 0"""
    x = np.array([-2.0, 0.0, 1.0, 3.0, np.nan])
    np.testing.assert_array_equal(hinge(x, 1.0), [0, 0, 0, 2, 0])
    np.testing.assert_array_equal(hinge(x, 1.0, side="below"), [3, 1, 0, 0, 0])
    np.testing.assert_array_equal(hinge(x, 1.0, 2), [0, 0, 0, 4, 0])
    np.testing.assert_array_equal(hinge(x, 1.0, 3, "below"), [27, 1, 0, 0, 0])
    np.testing.assert_array_equal(hinge(x, 1.0, 3), [0, 0, 0, 8, 0])
    # heating + cooling degree days: |x - k|; cooling - heating: x - k
    np.testing.assert_array_equal(hinge(x[:4], 1.0) - hinge(x[:4], 1.0, side="below"), x[:4] - 1.0)


KNOT_SETS = ([5.0, 15.0, 25.0], [0.0, 10.0, 20.0, 27.5, 35.0], [-3.0, 8.25, 19.0, 26.0, 31.5, 33.0, 40.0],
             [273.15 + v for v in (2.0, 12.0, 22.0, 30.0, 36.0)])


@pytest.mark.parametrize("knots", KNOT_SETS)
@pytest.mark.parametrize("normalize", [False, True])
def test_restated_spline_is_zero_below_and_linear_beyond(knots, normalize):
    """Every term is exactly 0 below t_1 (every cube is clamped away) and linear beyond t_K: its second difference on an equally
    spaced grid above t_K is 0 to the rounding of the cubes involved."""
    t = np.asarray(knots)
    K = len(t)
    lo = t[0] - np.arange(0.0, 40.0, 0.25)
    assert (rcspline_terms(lo, t, normalize) == 0).all()
    inside = rcspline_terms(np.linspace(t[0], t[-1], 50)[1:], t, normalize)
    assert inside.shape == (K - 2, 49) and (inside[0] > 0).all()                  # (not 0 everywhere)
    # the grid: t_K rounded up to a multiple of 1/4, then steps of 1/4 -- every x and every x +- h is exact in fp64
    h = 0.25
    x = np.ceil(t[-1] * 4 + 1) / 4 + h * np.arange(1, 200)
    f = rcspline_terms(np.stack([x - h, x, x + h]), t)                            # (K - 2, 3, len(x)), not normalised
    second = (f[:, 0] - 2.0 * f[:, 1]) + f[:, 2]
    ca, cb = rcspline_coefficients(t)
    # THE BOUND.  One evaluation of a term, with u = eps64 / 2 and M the largest of the three cube terms a^3, |ca| b^3, |cb| c^3
    # as they enter the sum:
    #   a^3:         the subtraction x - t_j rounds once (3u in the cube), two multiplications (2u)                  5 u M
    #   |ca| b^3:    the same cube (5u), the coefficient (two subtractions and a division: 3u), the product (1u)    9 u M
    #   |cb| c^3:    likewise                                                                                       9 u M
    #   two additions, of partial sums of at most 2 M and 3 M                                                       5 u M
    # = 28 u M = 14 eps64 M.  The second difference weighs three evaluations 1, 2, 1: 56 eps64 M; its own two additions (2 f is
    # exact) round sums of at most 6 M and 4 M: 10 u M = 5 eps64 M more.  COUNT = 61, rounded up to 64.
    COUNT = 64
    pts = np.stack([x - h, x, x + h])
    for j in range(K - 2):
        M = np.max([hinge(pts, t[j], 3), abs(ca[j]) * hinge(pts, t[-2], 3), abs(cb[j]) * hinge(pts, t[-1], 3)])
        bound = COUNT * EPS64 * M
        worst = np.abs(second[j]).max()
        print("knots %r term %d: largest second difference %.3g, bound %.3g, a cube's own %.3g" % (knots, j, worst, bound, 6 * h ** 3))
        assert worst <= bound and bound < 1e-3 * 6 * h ** 3                       # (a single cube's second difference is 6 h^2 (x - t) >> bound)
    if normalize:
        np.testing.assert_array_equal(rcspline_terms(x, t, True), rcspline_terms(x, t) / (t[-1] - t[0]) ** 2)
    # the slope beyond t_K, from the algebra: 3 * (t_K - t_j) * (t_{K-1} - t_j)
    slope = (f[:, 2] - f[:, 0]) / (2 * h)
    np.testing.assert_allclose(slope, np.broadcast_to((3 * (t[-1] - t[:-2]) * (t[-2] - t[:-2]))[:, None], slope.shape), rtol=1e-7)
