"""Temperature-bin day counts, the part that needs no GPU: the exports of wagg_bin_days_* (include/wagg.h), their bad-argument
codes (all decided before any device call), the workspace rule, the ceilT comparison rule as engine.bin_thresholds restates it,
and the argument checks of tas_bins_aggregate that precede any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_bin_days_reduce_f32", "wagg_bin_days_reduce_f64", "wagg_bin_days_work_bytes")


def test_exports_version_and_constants():
    """The three symbols are declared, bound and exported; the binding's constants are the header's; the version is 0.10.0."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, engine, seasons, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1000
    assert int(re.search(r"#define WAGG_BIN_EDGES_MAX (\d+)", header).group(1)) == _lib.BIN_EDGES_MAX == 65
    assert int(re.search(r"#define WAGG_BIN_GROUP (\d+)", header).group(1)) == _lib.BIN_GROUP
    assert 2 < _lib.BIN_GROUP < 15                             # (the GPU test's edge counts 3, G + 1, G + 2 and 17 are then distinct)
    assert callable(engine.bin_days_reduce) and callable(engine.bin_thresholds) and callable(seasons._bin_totals)
    assert pkg.tas_bins_aggregate is transformations.tas_bins_aggregate and "tas_bins_aggregate" in transformations.__all__


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, nothing dereferenced (every pointer below is a number no one may read)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)
    asc = (C.c_double * 66)(*range(66))

    def edges(*v):
        return (C.c_double * len(v))(*v)

    def call(fn, X=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win=p, offset=0.0, e=asc, n_edges=6, flags=0, out=p, ldo=8,
             pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, T, n, ldx, rb, rows, P, n_rows, doy, win, offset, e, n_edges, flags, out, ldo, pstride, status, work, work_bytes, None)

    inf, nan = float("inf"), float("nan")
    for fn in (L.wagg_bin_days_reduce_f32, L.wagg_bin_days_reduce_f64):
        for n_edges in (1, 66, 0, -1):
            assert call(fn, n_edges=n_edges) == -1 and b"n_edges must be 2..65" in L.wagg_last_error(), n_edges
        assert call(fn, e=None) == -1 and b"edges is NULL" in L.wagg_last_error()
        assert call(fn, e=edges(0.0, 2.0, 1.0), n_edges=3) == -1 and b"ascend strictly" in L.wagg_last_error()      # unsorted
        assert call(fn, e=edges(0.0, 1.0, 1.0), n_edges=3) == -1 and b"ascend strictly" in L.wagg_last_error()      # equal
        assert call(fn, e=edges(-inf, -inf, 1.0), n_edges=3) == -1 and b"ascend strictly" in L.wagg_last_error()
        assert call(fn, e=edges(0.0, nan, 2.0), n_edges=3) == -1 and b"NaN" in L.wagg_last_error()
        assert call(fn, e=edges(nan, 1.0), n_edges=2) == -1 and b"NaN" in L.wagg_last_error()
        assert call(fn, offset=nan) == -1 and call(fn, offset=inf) == -1 and b"offset" in L.wagg_last_error()
        assert call(fn, flags=64) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, flags=_lib.PERIOD_KEEP_NAN) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, doy=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        assert call(fn, win=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        for kw in ({"P": -1}, {"n": -3}, {"T": -1}, {"n_rows": -1}):
            assert call(fn, **kw) == -1 and b"negative size" in L.wagg_last_error(), kw
        assert call(fn, T=2 ** 31) == -1 and b"int32" in L.wagg_last_error()
        assert call(fn, ldx=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, ldo=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, pstride=15) == -1 and b"out_pstride smaller than P * ldo" in L.wagg_last_error()
        assert call(fn, status=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, rb=None) == -1 and call(fn, rows=None) == -1 and call(fn, out=None) == -1
        assert call(fn, X=None) == -1 and b"X_dev" in L.wagg_last_error()
        assert call(fn, work=C.c_void_p(0x1004), work_bytes=64) == -1 and call(fn, work_bytes=-8) == -1
        # nothing to do is not an error -- with or without a season, with open end bins -- and touches no device; one bin needs
        # no plane stride
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
        assert call(fn, P=0, doy=None, win=None) == 0
        assert call(fn, P=0, n_edges=65) == 0 and call(fn, P=0, e=edges(-inf, 0.0, inf), n_edges=3) == 0
        assert call(fn, n_edges=2, pstride=0, P=0, out=None) == 0


def test_work_bytes_are_the_period_kernels_for_the_bins():
    """0 for non-positive arguments and for fewer than two edges; otherwise what wagg_period_reduce_work_bytes reports for
    n_edges - 1 planes up to four bins (the same parts) and linear in the bins beyond."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    wb, period = L.wagg_bin_days_work_bytes, L.wagg_period_reduce_work_bytes
    for args in ((0, 1, 10, 3), (63, 0, 10, 3), (63, 1, 0, 3), (63, 1, 10, 1), (63, 1, 10, 0), (-1, 1, 10, 3), (63, 1, 10, -2)):
        assert wb(*args) == 0, args
    some = 0
    for n in (1, 63, 256, 1100, 24378, 1036800):
        for P in (1, 2, 3, 12, 70):
            for n_rows in (1, 9, 70, 365, 3650):
                for bins in (1, 2, 3, 4):
                    assert wb(n, P, n_rows, bins + 1) == period(n, P, n_rows, bins), (n, P, n_rows, bins)
                one = wb(n, P, n_rows, 2)
                some += one > 0
                for bins in (5, 8, 9, 17, 42, 64):
                    assert wb(n, P, n_rows, bins + 1) == bins * one, (n, P, n_rows, bins)
    assert some > 10 and wb(1100, 1, 70, 2) > 0 and wb(1036800, 12, 365, 43) == 0


def _around(f):
    """the float32 values around ``f``: two below, itself, two above (as far as there are any)"""
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    out = [f]
    with np.errstate(over="ignore"):                                              # (the step from the largest float to inf)
        for to in (lo, hi):
            x = f
            for _ in range(2):
                x = np.nextafter(x, to)
                out.append(x)
    return np.unique(np.asarray(out, dtype=np.float32))


def test_ceilT_rule():
    """x >= ceilT(c) exactly when float64(x) >= c, for 1,000 random fp64 c (magnitudes from subnormal to beyond the largest
    float) and the float32 values around each; for c exactly representable; for +-inf, zeros and subnormals; and with an
    offset (the thresholds of a Kelvin field).  fp64: ceilT(c) is c itself."""
    from climate_toolbox_amd import engine
    rng = np.random.default_rng(5)
    mant = rng.uniform(1.0, 2.0, 1000) * rng.choice([-1.0, 1.0], 1000)
    expo = np.concatenate([rng.integers(-20, 21, 700), rng.integers(-160, -120, 150), rng.integers(120, 135, 150)])
    c = np.concatenate([mant * 2.0 ** expo, rng.uniform(230.0, 330.0, 200)])
    exact = rng.standard_normal(100).astype(np.float32)
    tiny = np.float32(1e-45)                                                      # the smallest subnormal
    special = [np.inf, -np.inf, 0.0, -0.0, 1e-46, -1e-46, 1e-40, -1e-40, float(tiny), 1.5 * float(tiny), -0.5 * float(tiny),
               float(np.finfo(np.float32).max), 1e39, -1e39, float(np.finfo(np.float32).tiny), 273.15, -273.15]
    c = np.concatenate([c, exact.astype(np.float64), special])
    with np.errstate(over="ignore"):
        thr = engine.bin_thresholds(c, 0.0, np.float32)
    assert thr.dtype == np.float32 and thr.shape == c.shape and not np.isnan(thr).any()
    stepped = 0
    for ck, tk in zip(c, thr):
        with np.errstate(over="ignore"):
            near = np.float32(ck)
            below = np.nextafter(tk, np.float32(-np.inf))
        xs = np.unique(np.concatenate([_around(near), _around(tk), np.float32([0.0, -0.0, np.inf, -np.inf])]))
        np.testing.assert_array_equal(xs >= tk, xs.astype(np.float64) >= ck, err_msg="c = %r, ceilT = %r" % (ck, tk))
        assert float(tk) >= ck and (tk == -np.inf or float(below) < ck)           # the smallest such value
        stepped += float(near) < ck
    assert stepped > 300                                                          # (rounding to nearest came out below c: stepped up)
    np.testing.assert_array_equal(engine.bin_thresholds(exact.astype(np.float64), 0.0, np.float32), exact)
    assert engine.bin_thresholds([np.inf], 0.0, np.float32)[0] == np.inf and engine.bin_thresholds([-np.inf], 5.0, np.float32)[0] == -np.inf
    assert engine.bin_thresholds([1e39], 0.0, np.float32)[0] == np.inf
    assert engine.bin_thresholds([-1e39], 0.0, np.float32)[0] == -np.finfo(np.float32).max
    # with an offset: c = edge - offset in fp64, then rounded up
    e = np.arange(-5.0, 45.0, 0.5)
    k = engine.bin_thresholds(e, -273.15, np.float32)
    want = e + 273.15
    assert (k.astype(np.float64) >= want).all() and (np.nextafter(k, np.float32(-np.inf)).astype(np.float64) < want).all()
    np.testing.assert_array_equal(engine.bin_thresholds(e, -273.15, np.float64), want)
    with pytest.raises(TypeError):
        engine.bin_thresholds(e, 0.0, np.float16)


@pytest.mark.parametrize("bad", [[], (), [1.0], [1.0, 1.0], [2.0, 1.0], [0.0, 1.0, 0.5], [0.0, float("nan")], [float("-inf"), float("-inf"), 0.0],
                                 None, ["a", "b"], [[1.0, 2.0]]])
def test_edges_are_validated_before_any_device_work(bad):
    """Not even the dataset is looked at (None stands in for it)."""
    from climate_toolbox_amd import tas_bins_aggregate
    with pytest.raises(ValueError, match="edges"):
        tas_bins_aggregate(None, bad, "popwt", "hierid", {})


def _dataset():
    from climate_toolbox_amd import minixr
    tas = 280.0 + np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    return minixr.Dataset({"tas": (("time", "lat", "lon"), tas)},
                          coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})


def test_arguments_are_checked_before_any_device_work():
    """period=None (a bin count is a sum over days), season= without period=, cells and leap_days outside their values, a power
    and a degree-day variable: ValueError, with no GPU in sight."""
    from climate_toolbox_amd import minixr, tas_bins_aggregate
    from climate_toolbox_amd.transformations import tas_poly
    edges = [-np.inf, 0.0, 10.0, np.inf]
    with pytest.raises(ValueError, match="needs period="):
        tas_bins_aggregate(None, edges, "popwt", "hierid", {}, period=None)
    with pytest.raises(ValueError, match="season= needs period="):
        tas_bins_aggregate(None, edges, "popwt", "hierid", {}, period=None, season=object())
    with pytest.raises(ValueError, match="cells must be"):
        tas_bins_aggregate(None, edges, "popwt", "hierid", {}, cells="some")
    with pytest.raises(ValueError, match="leap_days"):
        tas_bins_aggregate(None, edges, "popwt", "hierid", {}, leap_days="maybe")
    ds = _dataset()
    powered = tas_poly(ds, 2, "tas-poly-2")
    with pytest.raises(ValueError, match="plain"):
        tas_bins_aggregate(powered, edges, "popwt", "hierid", {}, tas="tas-poly-2")
    tas = ds["tas"]
    ds["edd"] = minixr.LazyArray(tas.values, tas.dims, edd=(tas.values + 5.0, 0.0, [(1.0, 10.0)]), name="edd")
    with pytest.raises(ValueError, match="plain"):
        tas_bins_aggregate(ds, edges, "popwt", "hierid", {}, tas="edd")
    with pytest.raises(ValueError, match="time"):
        tas_bins_aggregate(minixr.Dataset({"tas": (("lat", "lon"), np.zeros((2, 4), dtype=np.float32))},
                                          coords={"lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5}), edges, "popwt", "hierid", {})
