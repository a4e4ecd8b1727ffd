"""Rolling-window extremes, the part that needs no GPU: the exports of wagg_rolling_* (include/wagg.h), their bad-argument codes
(all decided before any device call), the no-workspace rule, the argument checks of tas_rolling_aggregate that precede any device
work, and the NumPy restatement tests/rolling_ref.py against a brute-force np.max over explicitly enumerated windows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.rolling_ref import WIN_NULL, brute_force_max_mean, rolling_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_rolling_reduce_f32", "wagg_rolling_reduce_f64", "wagg_rolling_work_bytes")
T = 23
RB = np.array([0, 9, 17, 17])
ROWS = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17])


def test_exports_version_and_constants():
    """The three symbols are declared, bound and exported; the binding's constants are the header's; the version is 0.14.0."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, engine, seasons, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1400 and tuple(int(v) for v in pkg.__version__.split(".")) >= (0, 14, 0)
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))
    assert define("WAGG_ROLL_WINDOW_MAX") == _lib.ROLL_WINDOW_MAX == 16
    assert define("WAGG_ROLL_MAX_WINDOWS") == _lib.ROLL_MAX_WINDOWS == 8
    assert define("WAGG_ROLL_GROUP") == _lib.ROLL_GROUP >= 1
    assert (define("WAGG_ROLL_MAX"), define("WAGG_ROLL_MIN")) == (_lib.ROLL_MAX, _lib.ROLL_MIN) == (0, 1)
    assert (define("WAGG_ROLL_MEAN"), define("WAGG_ROLL_SUM")) == (_lib.ROLL_MEAN, _lib.ROLL_SUM) == (0, 1)
    assert callable(engine.rolling_reduce) and callable(seasons._rolling_totals)
    assert pkg.tas_rolling_aggregate is transformations.tas_rolling_aggregate and "tas_rolling_aggregate" in transformations.__all__


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, nothing dereferenced (every device pointer below is a number no one may read)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)

    def win(*v):
        return (C.c_int32 * len(v))(*v)

    some = win(1, 3, 5, 7, 16, 2, 3, 8)

    def call(fn, X=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win_=p, offset=0.0, w=some, n_win=4, stat=0, of=0, flags=0,
             out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, T, n, ldx, rb, rows, P, n_rows, doy, win_, offset, w, n_win, stat, of, flags, out, ldo, pstride, status, work,
                  work_bytes, None)

    inf, nan = float("inf"), float("nan")
    for fn in (L.wagg_rolling_reduce_f32, L.wagg_rolling_reduce_f64):
        for n_win in (0, 9, -1):
            assert call(fn, n_win=n_win) == -1 and b"n_win must be 1..8" in L.wagg_last_error(), n_win
        assert call(fn, w=None) == -1 and b"windows is NULL" in L.wagg_last_error()
        assert call(fn, w=win(1, 0, 2), n_win=3) == -1 and b"window 1 must be 1..16" in L.wagg_last_error()
        assert call(fn, w=win(17), n_win=1) == -1 and b"window 0 must be 1..16" in L.wagg_last_error()
        assert call(fn, w=win(3, 4, -2), n_win=3) == -1 and b"window 2 must be 1..16" in L.wagg_last_error()
        assert call(fn, offset=nan) == -1 and call(fn, offset=inf) == -1 and b"offset must be finite" in L.wagg_last_error()
        for bad in (-1, 2, 17):
            assert call(fn, stat=bad) == -1 and b"stat must be" in L.wagg_last_error(), bad
            assert call(fn, of=bad) == -1 and b"of must be" in L.wagg_last_error(), bad
        assert call(fn, flags=64) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, flags=_lib.PERIOD_KEEP_NAN) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, doy=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        assert call(fn, win_=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        for kw in ({"P": -1}, {"n": -3}, {"T": -1}, {"n_rows": -1}):
            assert call(fn, **kw) == -1 and b"negative size" in L.wagg_last_error(), kw
        assert call(fn, T=2 ** 31) == -1 and b"int32" in L.wagg_last_error()
        assert call(fn, ldx=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, ldo=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, pstride=15) == -1 and b"out_pstride smaller than P * ldo" in L.wagg_last_error()
        assert call(fn, status=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, rb=None) == -1 and call(fn, rows=None) == -1 and call(fn, out=None) == -1
        assert call(fn, X=None) == -1 and b"X_dev" in L.wagg_last_error()
        # nothing to do is not an error -- with or without a season, either extreme of either quantity, unsorted windows with a
        # duplicate -- and touches no device; one window needs no plane stride; the workspace arguments are not looked at
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
        assert call(fn, P=0, doy=None, win_=None) == 0
        assert call(fn, P=0, n_win=8) == 0 and call(fn, P=0, w=win(16, 1, 16), n_win=3) == 0
        assert call(fn, P=0, stat=_lib.ROLL_MIN, of=_lib.ROLL_SUM, offset=-273.15) == 0
        assert call(fn, n_win=1, pstride=0, P=0, out=None) == 0
        assert call(fn, P=0, work=C.c_void_p(0x1004), work_bytes=-8) == 0


def test_no_workspace():
    """A window does not add across the parts of a list: the family never splits one, and asks for no scratch."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    for n in (0, 1, 63, 1100, 24378, 1036800):
        for P in (0, 1, 12, 70):
            for n_rows in (0, 9, 365, 36500):
                for n_win in (0, 1, 4, 8):
                    assert L.wagg_rolling_work_bytes(n, P, n_rows, n_win) == 0
    assert L.wagg_bin_days_work_bytes(1100, 1, 365, 2) > 0        # (where the bins would split)


@pytest.mark.parametrize("bad", [[0], [17], [2.5], [True], [], (), [3, 0], [1, 17], [np.float32(2)], ["3"], [None], None, 5, [-1], [np.True_]])
def test_windows_are_validated_before_any_device_work(bad):
    """window 0, 17, 2.5, True, an empty list ...: not even the dataset is looked at (None stands in for it)."""
    from climate_toolbox_amd import tas_rolling_aggregate
    with pytest.raises(ValueError, match="windows"):
        tas_rolling_aggregate(None, bad, "popwt", "hierid", {})


def test_arguments_are_checked_before_any_device_work():
    """stat, of; period=None, cells, leap_days; a power variable: ValueError, with no GPU in sight."""
    from climate_toolbox_amd import minixr, tas_rolling_aggregate
    from climate_toolbox_amd.transformations import tas_poly
    w = [5, 1, 16, 5, np.int64(3)]
    for bad in ("mean", "maximum", None, 0):
        with pytest.raises(ValueError, match="stat must be"):
            tas_rolling_aggregate(None, w, "popwt", "hierid", {}, stat=bad)
    for bad in ("max", "average", None, 1):
        with pytest.raises(ValueError, match="of must be"):
            tas_rolling_aggregate(None, w, "popwt", "hierid", {}, of=bad)
    for kw in ({}, {"stat": "min", "of": "sum"}):
        with pytest.raises(ValueError, match="needs period="):
            tas_rolling_aggregate(None, w, "popwt", "hierid", {}, period=None, **kw)
    with pytest.raises(ValueError, match="season= needs period="):
        tas_rolling_aggregate(None, w, "popwt", "hierid", {}, period=None, season=object())
    with pytest.raises(ValueError, match="cells must be"):
        tas_rolling_aggregate(None, w, "popwt", "hierid", {}, cells="some")
    with pytest.raises(ValueError, match="leap_days"):
        tas_rolling_aggregate(None, w, "popwt", "hierid", {}, leap_days="maybe")
    tas = 280.0 + np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    ds = minixr.Dataset({"tas": (("time", "lat", "lon"), tas)},
                        coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})
    with pytest.raises(ValueError, match="plain"):
        tas_rolling_aggregate(tas_poly(ds, 2, "tas-poly-2"), w, "popwt", "hierid", {}, tas="tas-poly-2")
    with pytest.raises(ValueError, match="time"):
        tas_rolling_aggregate(minixr.Dataset({"tas": (("lat", "lon"), np.zeros((2, 4), dtype=np.float32))},
                                             coords={"lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5}), w, "popwt", "hierid", {})


def test_engine_arguments_are_checked_before_any_device_work():
    """engine.rolling_reduce checks X first, which a host array fails."""
    from climate_toolbox_amd import engine
    with pytest.raises((TypeError, ValueError)):
        engine.rolling_reduce(np.zeros((3, 4), dtype=np.float32), [0, 3], [0, 1, 2], 0.0, [1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_equals_brute_force_over_enumerated_windows(dtype):
    """Small integers (every sum is exact in any order), the spells' small shape: a gap inside period 0, rows 9 | 10 consecutive
    across the period boundary, 8 entries in period 1, period 2 empty.  max / mean against np.max over the enumerated windows;
    min = -max(-x); sum = W * mean; the offset is added once (W times for a sum)."""
    rng = np.random.default_rng(5)
    X = rng.integers(-40, 41, (T, 37)).astype(dtype)
    lengths = [1, 2, 3, 4, 5, 8, 9, 16]
    got = rolling_ref(X, RB, ROWS, 0.0, lengths)
    assert got.dtype == dtype and got.shape == (8, 3, 37)
    for k, W in enumerate(lengths):
        want = brute_force_max_mean(X, RB, ROWS, W).astype(dtype)
        np.testing.assert_array_equal(got[k], want)
        np.testing.assert_array_equal(rolling_ref(X, RB, ROWS, 0.0, [W], stat="min")[0], -brute_force_max_mean(-X, RB, ROWS, W).astype(dtype))
        np.testing.assert_array_equal(rolling_ref(X, RB, ROWS, 0.0, [W], of="sum")[0], (brute_force_max_mean(X, RB, ROWS, W) * W).astype(dtype))
        np.testing.assert_array_equal(rolling_ref(X, RB, ROWS, 2.0, [W], of="sum")[0],
                                      (brute_force_max_mean(X, RB, ROWS, W) * W + 2.0 * W).astype(dtype))
    assert np.isnan(got[:, 2]).all()                                             # the empty period
    assert np.isnan(got[6:, :2]).all() and not np.isnan(got[:5, :2]).any()       # 9 > 4 | 5 and > 8; 5 fits behind the gap ...
    assert np.isnan(got[5, 0]).all() and not np.isnan(got[5, 1]).any()           # ... and 8 fits period 1 only


def test_ref_by_hand():
    """one cell, rows 0..5: 1 5 2 NaN 4 3.  W = 2: windows (1 5) (5 2) (4 3) -> max 3.5, min 3; W = 3: (1 5 2) only; W = 4: none.
    A season that leaves out day 1 leaves W = 2 with (4 3) only.  Strict compares keep the first of two equal sums."""
    X = np.array([[1.0, 5.0, 2.0, np.nan, 4.0, 3.0]]).T
    rb, rows = [0, 6], np.arange(6)
    out = rolling_ref(X, rb, rows, 0.0, [1, 2, 3, 4])
    assert out[:3, 0, 0].tolist() == [5.0, 3.5, 8.0 / 3.0] and np.isnan(out[3, 0, 0])
    assert rolling_ref(X, rb, rows, 0.0, [2, 3], stat="min", of="sum")[:, 0, 0].tolist() == [6.0, 8.0]
    assert rolling_ref(X, rb, rows, -1.0, [2], of="sum")[0, 0, 0] == 5.0 and rolling_ref(X, rb, rows, -1.0, [2])[0, 0, 0] == 2.5
    doy = np.arange(10, 16)
    win = np.array([12 | 15 << 10])
    assert rolling_ref(X, rb, rows, 0.0, [1, 2], doy=doy, windows=win)[:, 0, 0].tolist() == [4.0, 3.5]
    assert np.isnan(rolling_ref(X, rb, rows, 0.0, [1], doy=doy, windows=np.array([WIN_NULL]))).all()
    assert rolling_ref(X, [0, 3, 6], rows, 0.0, [2])[0, :, 0].tolist() == [3.5, 3.5]        # (5 2) | (4 3): never (2 NaN) or (2 4)
    assert rolling_ref(X, [0, 5], [0, 1, 2, 4, 5], 0.0, [2])[0, 0, 0] == 3.5               # row 3 dropped: (2 4) is no window
    inf = np.array([[1.0, np.inf, -np.inf, 2.0]]).T                                        # inf - inf is NaN: never taken
    assert rolling_ref(inf, [0, 4], np.arange(4), 0.0, [2])[0, 0, 0] == np.inf
    assert rolling_ref(inf, [0, 4], np.arange(4), 0.0, [2], stat="min")[0, 0, 0] == -np.inf
