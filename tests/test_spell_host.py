"""Spell statistics, the part that needs no GPU: the exports of wagg_spell_* (include/wagg.h), their bad-argument codes (all
decided before any device call), the no-workspace rule, the argument checks of tas_spell_aggregate that precede any device work,
and the NumPy restatement tests/spell_ref.py against cases worked out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.spell_ref import WIN_INVERT, WIN_NULL, spell_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_spell_reduce_f32", "wagg_spell_reduce_f64", "wagg_spell_work_bytes")


def test_exports_version_and_constants():
    """The three symbols are declared, bound and exported; the binding's constants are the header's; the version is 0.13.0."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, engine, seasons, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1300 and tuple(int(v) for v in pkg.__version__.split(".")) >= (0, 13, 0)
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))
    assert define("WAGG_SPELL_MAX") == _lib.SPELL_MAX == 64
    assert define("WAGG_SPELL_GROUP") == _lib.SPELL_GROUP and 2 < _lib.SPELL_GROUP < 32 and _lib.SPELL_MAX % _lib.SPELL_GROUP == 0
    assert define("WAGG_SPELL_MIN_LENGTH_MAX") == _lib.SPELL_MIN_LENGTH_MAX == 32767
    assert (define("WAGG_SPELL_DAYS"), define("WAGG_SPELL_EVENTS"), define("WAGG_SPELL_LONGEST")) == \
        (_lib.SPELL_DAYS, _lib.SPELL_EVENTS, _lib.SPELL_LONGEST) == (0, 1, 2)
    assert callable(engine.spell_reduce) and callable(seasons._spell_totals)
    assert pkg.tas_spell_aggregate is transformations.tas_spell_aggregate and "tas_spell_aggregate" in transformations.__all__


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, nothing dereferenced (every pointer below is a number no one may read)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)
    some = (C.c_double * 65)(*range(65))

    def thr(*v):
        return (C.c_double * len(v))(*v)

    def call(fn, X=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win=p, offset=0.0, t=some, n_thr=5, L_=3, stat=0, below=0,
             flags=0, out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, T, n, ldx, rb, rows, P, n_rows, doy, win, offset, t, n_thr, L_, stat, below, flags, out, ldo, pstride, status, work,
                  work_bytes, None)

    inf, nan = float("inf"), float("nan")
    for fn in (L.wagg_spell_reduce_f32, L.wagg_spell_reduce_f64):
        for n_thr in (0, 65, -1):
            assert call(fn, n_thr=n_thr) == -1 and b"n_thr must be 1..64" in L.wagg_last_error(), n_thr
        assert call(fn, t=None) == -1 and b"thresholds is NULL" in L.wagg_last_error()
        assert call(fn, t=thr(0.0, nan, 2.0), n_thr=3) == -1 and b"threshold 1 is NaN" in L.wagg_last_error()
        assert call(fn, t=thr(inf, 1.0), n_thr=2) == -1 and b"threshold 0 is infinite" in L.wagg_last_error()
        assert call(fn, t=thr(0.0, 1.0, -inf), n_thr=3) == -1 and b"threshold 2 is infinite" in L.wagg_last_error()
        assert call(fn, offset=nan) == -1 and call(fn, offset=inf) == -1 and b"offset must be finite" in L.wagg_last_error()
        for bad in (0, -1, 32768, 2 ** 31 - 1):
            assert call(fn, L_=bad) == -1 and b"min_length must be 1..32767" in L.wagg_last_error(), bad
        for bad in (-1, 3, 17):
            assert call(fn, stat=bad, L_=1) == -1 and b"stat must be" in L.wagg_last_error(), bad
        assert call(fn, stat=_lib.SPELL_LONGEST, L_=2) == -1 and b"WAGG_SPELL_LONGEST does not use min_length" in L.wagg_last_error()
        for bad in (-1, 2):
            assert call(fn, below=bad) == -1 and b"below must be 0 or 1" in L.wagg_last_error(), bad
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
        # nothing to do is not an error -- with or without a season, for every statistic and side, unsorted thresholds with a
        # duplicate -- and touches no device; one threshold needs no plane stride; the workspace arguments are not looked at
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
        assert call(fn, P=0, doy=None, win=None) == 0
        assert call(fn, P=0, n_thr=64) == 0 and call(fn, P=0, t=thr(3.0, -1.0, 3.0), n_thr=3) == 0
        assert call(fn, P=0, L_=32767) == 0 and call(fn, P=0, L_=1, stat=_lib.SPELL_LONGEST, below=1) == 0
        assert call(fn, P=0, stat=_lib.SPELL_EVENTS) == 0
        assert call(fn, n_thr=1, pstride=0, P=0, out=None) == 0
        assert call(fn, P=0, work=C.c_void_p(0x1004), work_bytes=-8) == 0


def test_no_workspace():
    """A run does not add across the parts of a list: the family never splits one, and asks for no scratch."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    for n in (0, 1, 63, 1100, 24378, 1036800):
        for P in (0, 1, 12, 70):
            for n_rows in (0, 9, 365, 36500):
                for n_thr in (0, 1, 8, 9, 64):
                    assert L.wagg_spell_work_bytes(n, P, n_rows, n_thr) == 0
    assert L.wagg_bin_days_work_bytes(1100, 1, 365, 2) > 0        # (where the bins would split)


@pytest.mark.parametrize("bad", [[], (), None, 35.0, ["a"], [[30.0, 35.0]], [30.0, float("nan")], [float("inf")], [float("-inf"), 30.0]])
def test_thresholds_are_validated_before_any_device_work(bad):
    """Not even the dataset is looked at (None stands in for it)."""
    from climate_toolbox_amd import tas_spell_aggregate
    with pytest.raises(ValueError, match="thresholds"):
        tas_spell_aggregate(None, bad, "popwt", "hierid", {})


def _dataset():
    from climate_toolbox_amd import minixr
    tas = 280.0 + np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    return minixr.Dataset({"tas": (("time", "lat", "lon"), tas)},
                          coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})


def test_arguments_are_checked_before_any_device_work():
    """min_length, stat, side; period=None, cells, leap_days; a power and a degree-day variable: ValueError, with no GPU in sight."""
    from climate_toolbox_amd import minixr, tas_spell_aggregate
    from climate_toolbox_amd.transformations import tas_poly
    thr = [35.0, 30.0, 35.0]
    for bad in (0, -1, 32768, 2.0, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="min_length"):
            tas_spell_aggregate(None, thr, "popwt", "hierid", {}, min_length=bad)
    with pytest.raises(ValueError, match="stat must be"):
        tas_spell_aggregate(None, thr, "popwt", "hierid", {}, stat="count")
    with pytest.raises(ValueError, match="side must be"):
        tas_spell_aggregate(None, thr, "popwt", "hierid", {}, side="over")
    for bad in (2, 4, 32767):
        with pytest.raises(ValueError, match="longest"):
            tas_spell_aggregate(None, thr, "popwt", "hierid", {}, stat="longest", min_length=bad)
    for fine in ({}, {"min_length": 1}, {"min_length": 3}):       # (the default counts as unset: the next check is reached)
        with pytest.raises(ValueError, match="needs period="):
            tas_spell_aggregate(None, thr, "popwt", "hierid", {}, stat="longest", period=None, **fine)
    with pytest.raises(ValueError, match="needs period="):
        tas_spell_aggregate(None, thr, "popwt", "hierid", {}, period=None)
    with pytest.raises(ValueError, match="season= needs period="):
        tas_spell_aggregate(None, thr, "popwt", "hierid", {}, period=None, season=object())
    with pytest.raises(ValueError, match="cells must be"):
        tas_spell_aggregate(None, thr, "popwt", "hierid", {}, cells="some")
    with pytest.raises(ValueError, match="leap_days"):
        tas_spell_aggregate(None, thr, "popwt", "hierid", {}, leap_days="maybe")
    ds = _dataset()
    powered = tas_poly(ds, 2, "tas-poly-2")
    with pytest.raises(ValueError, match="plain"):
        tas_spell_aggregate(powered, thr, "popwt", "hierid", {}, tas="tas-poly-2")
    tas = ds["tas"]
    ds["edd"] = minixr.LazyArray(tas.values, tas.dims, edd=(tas.values + 5.0, 0.0, [(1.0, 10.0)]), name="edd")
    with pytest.raises(ValueError, match="plain"):
        tas_spell_aggregate(ds, thr, "popwt", "hierid", {}, tas="edd")
    with pytest.raises(ValueError, match="time"):
        tas_spell_aggregate(minixr.Dataset({"tas": (("lat", "lon"), np.zeros((2, 4), dtype=np.float32))},
                                           coords={"lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5}), thr, "popwt", "hierid", {})


def test_engine_arguments_are_checked_before_any_device_work():
    """engine.spell_reduce: thresholds, stat, side, min_length -- behind the check of X, which a host array fails first."""
    from climate_toolbox_amd import engine
    with pytest.raises((TypeError, ValueError)):
        engine.spell_reduce(np.zeros((3, 4), dtype=np.float32), [0, 3], [0, 1, 2], 0.0, [1.0])


# ---- spell_ref against cases worked out by hand: one cell per column, one period unless said otherwise --------------------------
def _all(X, row_begin, rows, L, **kw):
    X = np.asarray(X, dtype=np.float64)
    return tuple(spell_ref(X, row_begin, rows, 0.0, [1.0], L if stat != "longest" else 1, stat, **kw)[0].astype(int).tolist()
                 for stat in ("days", "events", "longest"))


def test_ref_run_of_exactly_L_and_of_L_minus_1():
    """columns: a run of exactly 3; a run of 2; 1 1 0 1 1 1 0 1 (runs of 2, 3 and 1)"""
    X = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 0], [1, 1, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1]])
    rb, rows = [0, 8], np.arange(8)
    assert _all(X, rb, rows, 3) == ([[3, 0, 3]], [[1, 0, 1]], [[3, 2, 3]])
    assert _all(X, rb, rows, 2) == ([[3, 2, 5]], [[1, 1, 2]], [[3, 2, 3]])
    assert _all(X, rb, rows, 1) == ([[3, 2, 6]], [[1, 1, 3]], [[3, 2, 3]])
    assert _all(X, rb, rows, 4) == ([[0, 0, 0]], [[0, 0, 0]], [[3, 2, 3]])
    # below: the cold days of the same field (thresholds compare x < 1)
    assert _all(X, rb, rows, 2, side="below") == ([[4, 6, 0]], [[1, 2, 0]], [[4, 4, 1]])


def test_ref_run_cut_by_a_row_gap():
    """six hot entries, rows 0 1 2 | 4 5 6 (row 3 dropped): two runs of 3, not one of 6; rows that repeat or descend cut too"""
    X = np.ones((8, 1))
    assert _all(X, [0, 6], [0, 1, 2, 4, 5, 6], 3) == ([[6]], [[2]], [[3]])
    assert _all(X, [0, 6], [0, 1, 2, 4, 5, 6], 4) == ([[0]], [[0]], [[3]])
    assert _all(X, [0, 6], [0, 1, 2, 3, 4, 5], 4) == ([[6]], [[1]], [[6]])
    assert _all(X, [0, 4], [2, 2, 3, 1], 1) == ([[4]], [[3]], [[2]])
    assert _all(X, [0, 3], [0, 9, 1], 1) == ([[2]], [[2]], [[1]])                # a row outside the field is cold


def test_ref_run_cut_by_a_period_boundary():
    """hot on rows 2..6, periods rows 0..3 and 4..7: 2 + 3 days, never a run of 5; an empty period is all zero"""
    X = np.zeros((8, 1))
    X[2:7] = 1
    rows = np.arange(8)
    assert _all(X, [0, 4, 8, 8], rows, 1) == ([[2], [3], [0]], [[1], [1], [0]], [[2], [3], [0]])
    assert _all(X, [0, 4, 8, 8], rows, 3) == ([[0], [3], [0]], [[0], [1], [0]], [[2], [3], [0]])
    assert _all(X, [0, 8], rows, 5) == ([[5]], [[1]], [[5]])


def test_ref_run_cut_by_a_season_boundary_and_by_an_inverted_window():
    """eight hot days of year 10..17.  Cells: all year; in season 10..13 (a run of 4); 12..14 (3); the complement of [12, 14] (2 + 3:
    the window's own ends are out); null; a window that holds none of the days"""
    X = np.ones((8, 6))
    doy = np.arange(10, 18)
    win = np.array([0 | 1023 << 10, 10 | 13 << 10, 12 | 14 << 10, 12 | 14 << 10 | WIN_INVERT, 1 | 0 << 10 | WIN_NULL, 100 | 200 << 10])
    kw = dict(doy=doy, windows=win)
    assert _all(X, [0, 8], np.arange(8), 1, **kw) == ([[8, 4, 3, 5, 0, 0]], [[1, 1, 1, 2, 0, 0]], [[8, 4, 3, 3, 0, 0]])
    assert _all(X, [0, 8], np.arange(8), 3, **kw) == ([[8, 4, 3, 3, 0, 0]], [[1, 1, 1, 1, 0, 0]], [[8, 4, 3, 3, 0, 0]])
    doy2 = doy.copy()
    doy2[3] = 2000                                                                # a day of year outside 0..1023 is in no season
    assert _all(X[:, :1], [0, 8], np.arange(8), 1, doy=doy2, windows=win[:1]) == ([[7]], [[2]], [[4]])


def test_ref_nan_inside_a_run():
    """1 1 NaN 1 1 1: NaN is cold on either side, it cuts the run; +inf is hot above, -inf hot below"""
    X = np.array([[1.0, 1.0, np.nan, 1.0, 1.0, 1.0], [0.0, 0.0, np.nan, 0.0, 0.0, 0.0], [1.0, np.inf, 1.0, -np.inf, 1.0, 1.0]]).T
    assert _all(X, [0, 6], np.arange(6), 1) == ([[5, 0, 5]], [[2, 0, 2]], [[3, 0, 3]])
    assert _all(X, [0, 6], np.arange(6), 1, side="below") == ([[0, 5, 1]], [[0, 2, 1]], [[0, 3, 1]])
    assert _all(X, [0, 6], np.arange(6), 3) == ([[3, 0, 3]], [[1, 0, 1]], [[3, 0, 3]])


def test_ref_offset_and_thresholds_are_independent_planes():
    """float64(x) + offset against every threshold, in the caller's order, duplicates included"""
    X = (np.array([[20.0, 31.0, 36.0, 36.0, 29.0, 41.0]]).T + 273.15).astype(np.float32)
    got = spell_ref(X, [0, 6], np.arange(6), -273.15, [35.0, 30.0, 35.0, 50.0], 2, "days")
    assert got[:, 0, 0].tolist() == [2.0, 3.0, 2.0, 0.0] and got.dtype == np.float64
