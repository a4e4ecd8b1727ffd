"""Spells against per-cell thresholds, the part that needs no GPU: the exports of wagg_cell_spells_* (include/wagg.h) and their
names' place among the row-list families, their bad-argument codes (all decided before any device call), the NumPy restatement
tests/cell_spell_ref.py against tests/spell_ref.py and cases worked out by hand, how tas_relative_spell_aggregate matches periods
to planes, and the shapes CellThresholds.from_array takes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.cell_spell_ref import cell_spell_ref
from tests.spell_ref import spell_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_cell_spells_f32", "wagg_cell_spells_f64")


def test_exports_version_and_constants():
    """The two symbols are declared, bound and exported; the binding's constants are the header's; the version is 0.16.0."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, relative, seasons, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1600 and tuple(int(v) for v in pkg.__version__.split(".")) >= (0, 16, 0)
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))
    assert define("WAGG_CELL_SPELL_MAX") == _lib.CELL_SPELL_MAX == 64
    assert define("WAGG_CELL_SPELL_GROUP") == _lib.CELL_SPELL_GROUP and _lib.CELL_SPELL_GROUP in (4, 8)
    assert (define("WAGG_CELL_SPELL_AMOUNT"), define("WAGG_CELL_SPELL_EXCESS")) == (_lib.CELL_SPELL_AMOUNT, _lib.CELL_SPELL_EXCESS)
    assert len({_lib.SPELL_DAYS, _lib.SPELL_EVENTS, _lib.SPELL_LONGEST, _lib.CELL_SPELL_AMOUNT, _lib.CELL_SPELL_EXCESS}) == 5
    assert callable(relative.cell_spell_reduce) and callable(relative.cell_quantiles) and callable(seasons._cell_spell_totals)
    assert pkg.tas_relative_spell_aggregate is transformations.tas_relative_spell_aggregate
    assert "tas_relative_spell_aggregate" in transformations.__all__ and pkg.CellThresholds is relative.CellThresholds


def test_export_names_stay_out_of_the_other_families_patterns():
    """The guards of the layout, quantile and spell host tests go by name: these exports are no ``*_reduce_*`` / ``*_select_*``
    entry point, do not speak of quantiles, and the family has no work-size query."""
    from climate_toolbox_amd import _lib
    family = [n for n in _lib.EXPORTS if n.startswith("wagg_cell_")]
    assert sorted(family) == sorted(NAMES), family                   # (what the binding lists for this family, not a literal)
    for name in family:
        assert not re.fullmatch(r"wagg_\w+_(reduce|select)_(f32|f64)", name) and "quantile" not in name and not name.endswith("_work_bytes")
    assert not [n for n in _lib.EXPORTS if n.startswith("wagg_cell") and n.endswith("_work_bytes")]
    # the device-level call is not an engine callable: the stream tables of the engine's own tests stay as they are
    from climate_toolbox_amd import engine
    assert not hasattr(engine, "cell_spell_reduce")


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, nothing dereferenced (every pointer below is a number no one may read)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)

    def call(fn, X=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win=p, offset=0.0, thr=p, n_thr=5, ldt=8, kstride=16,
             pmap=p, M=2, L_=3, stat=0, below=0, flags=0, out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, T, n, ldx, rb, rows, P, n_rows, doy, win, offset, thr, n_thr, ldt, kstride, pmap, M, L_, stat, below, flags, out, ldo,
                  pstride, status, work, work_bytes, None)

    inf, nan = float("inf"), float("nan")
    for fn in (L.wagg_cell_spells_f32, L.wagg_cell_spells_f64):
        for n_thr in (0, 65, -1):
            assert call(fn, n_thr=n_thr) == -1 and b"n_thr must be 1..64" in L.wagg_last_error(), n_thr
        for M in (0, -1):
            assert call(fn, M=M) == -1 and b"M must be at least 1" in L.wagg_last_error(), M
        assert call(fn, thr=None) == -1 and b"thr_dev is NULL" in L.wagg_last_error()
        assert call(fn, ldt=7) == -1 and b"ldt smaller than n" in L.wagg_last_error()
        assert call(fn, kstride=15) == -1 and b"thr_kstride smaller than M * ldt" in L.wagg_last_error()
        assert call(fn, M=3, kstride=23) == -1 and b"thr_kstride smaller than M * ldt" in L.wagg_last_error()
        assert call(fn, ldt=2 ** 62, kstride=2 ** 62) == -1 and b"thr_kstride smaller than M * ldt" in L.wagg_last_error()
        # a NULL map: one plane, or one plane per period -- nothing else
        assert call(fn, pmap=None, M=3, kstride=24) == -1 and b"plane_of_period_dev is NULL" in L.wagg_last_error()
        assert call(fn, pmap=None, M=3, kstride=24, P=4, pstride=32) == -1 and b"M == 1 or M == P" in L.wagg_last_error()
        assert call(fn, offset=nan) == -1 and call(fn, offset=inf) == -1 and b"offset must be finite" in L.wagg_last_error()
        for bad in (0, -1, 32768):
            assert call(fn, L_=bad) == -1 and b"min_length must be 1..32767" in L.wagg_last_error(), bad
        for bad in (-1, 5, 17):
            assert call(fn, stat=bad, L_=1) == -1 and b"stat must be" in L.wagg_last_error(), bad
        assert call(fn, stat=_lib.SPELL_LONGEST, L_=2) == -1 and b"WAGG_SPELL_LONGEST does not use min_length" in L.wagg_last_error()
        for stat in (_lib.CELL_SPELL_AMOUNT, _lib.CELL_SPELL_EXCESS):
            for bad in (2, 3, 6):
                assert call(fn, stat=stat, L_=bad) == -1 and b"min_length must be 1" in L.wagg_last_error(), (stat, bad)
        for bad in (-1, 2):
            assert call(fn, below=bad) == -1 and b"below must be 0 or 1" in L.wagg_last_error(), bad
        assert call(fn, flags=64) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, flags=_lib.PERIOD_KEEP_NAN) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, doy=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        for kw in ({"P": -1}, {"n": -3}, {"T": -1}, {"n_rows": -1}):
            assert call(fn, **kw) == -1 and b"negative size" in L.wagg_last_error(), kw
        assert call(fn, ldx=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, pstride=15) == -1 and b"out_pstride smaller than P * ldo" in L.wagg_last_error()
        assert call(fn, status=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, rb=None) == -1 and call(fn, rows=None) == -1 and call(fn, out=None) == -1
        assert call(fn, X=None) == -1 and b"X_dev" in L.wagg_last_error()
        # nothing to do is not an error and touches no device: every statistic and side, a NULL map for M == 1 and for M == P (= 0
        # here), one level without a plane stride, the workspace arguments not looked at
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, ldt=0, kstride=0, out=None, X=None) == 0
        assert call(fn, P=0, doy=None, win=None) == 0 and call(fn, P=0, n_thr=64) == 0
        assert call(fn, P=0, pmap=None, M=1) == 0 and call(fn, P=2, n=0, ldx=0, ldo=0, ldt=0, kstride=0, pmap=None, M=2) == 0
        for stat in (_lib.SPELL_EVENTS, _lib.SPELL_LONGEST, _lib.CELL_SPELL_AMOUNT, _lib.CELL_SPELL_EXCESS):
            assert call(fn, P=0, stat=stat, L_=1, below=1) == 0, stat
        assert call(fn, P=0, n_thr=1, M=1, kstride=8, pstride=0, out=None) == 0
        assert call(fn, P=0, work=C.c_void_p(0x1004), work_bytes=-8) == 0


T, RB = 23, np.array([0, 9, 17, 17])
ROWS = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17])


def _field(n, dtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 10.0, (T, n))
    X[:, ::2] = np.where(rng.uniform(size=(T, (n + 1) // 2)) < 0.8, 8.5, 1.5)
    X[4, 1 % n] = np.nan
    return X.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constant_threshold_field_is_the_scalar_restatement(dtype):
    """All three counts, both sides, with and without a season and a Kelvin offset: a threshold field that is the same number in
    every cell gives tests/spell_ref.py's counts."""
    n = 13
    X = _field(n, dtype, 3)
    thr = np.array([5.0, 2.0, 8.75])
    field = np.broadcast_to(thr.astype(dtype)[:, None, None], (3, 1, n))
    doy = np.arange(100, 100 + T)
    win = np.where(np.arange(n) % 3 == 0, 0 | 1023 << 10, 101 | 112 << 10).astype(np.int32)
    for kw in ({}, dict(doy=doy, windows=win)):
        for side in ("above", "below"):
            for stat, L in (("days", 1), ("days", 3), ("events", 2), ("longest", 1)):
                got = cell_spell_ref(X, RB, ROWS, 0.0, field, None, L, stat, side, **kw)
                np.testing.assert_array_equal(got, spell_ref(X, RB, ROWS, 0.0, thr, L, stat, side, **kw), (side, stat, L))
    Xk = (X + dtype(273.15)).astype(dtype)
    got = cell_spell_ref(Xk, RB, ROWS, -273.15, field, None, 2, "days", "above")
    np.testing.assert_array_equal(got, spell_ref(Xk, RB, ROWS, -273.15, thr.astype(dtype).astype(np.float64), 2, "days", "above"))


def test_restatement_by_hand():
    """One cell, rows 0..5 in one period without row 3: values 1 5 9 | 9 2 against thresholds 4 (plane 0) and 9 (plane 1); the
    plane map, the NaN threshold, an out-of-range plane, and the two sums in list order."""
    X = np.array([[1.0], [5.0], [9.0], [7.0], [9.0], [2.0]])
    rb, rows = np.array([0, 5, 5]), np.array([0, 1, 2, 4, 5])
    thr = np.array([[[4.0], [9.0]], [[np.nan], [-np.inf]]])                      # (K = 2, M = 2, n = 1)
    ref = lambda pmap, **kw: cell_spell_ref(X, rb, rows, 0.0, thr, pmap, **kw)[:, :, 0]
    days = ref([0, 1])
    assert days[0].tolist() == [3.0, 0.0] and np.isnan(days[1, 0]) and days[1, 1] == 0.0          # 5 9 | 9 hot; the empty period
    assert ref([1, 0])[:, 0].tolist() == [2.0, 5.0]                                             # 9 | 9; everything above -inf
    assert ref([1, 0], stat="longest")[:, 0].tolist() == [1.0, 3.0]                             # the gap cuts 1 5 9 | 9 2
    assert ref([1, 0], stat="events", min_length=2)[:, 0].tolist() == [0.0, 2.0]
    assert ref([0, 0], stat="amount")[0].tolist() == [23.0, 0.0]
    assert ref([0, 0], stat="excess")[0].tolist() == [11.0, 0.0] and ref([0, 0], stat="excess", side="below")[0].tolist() == [5.0, 0.0]
    assert ref([1, 0], stat="excess")[1, 0] == np.inf
    out = ref([2, -1])
    assert np.isnan(out).all()
    assert ref(None)[0].tolist() == [3.0, 0.0]                                                  # M == P: period p reads plane p
    # the sums are sequential fp64 additions: 1e16 + 1 + 1 loses both ones, 1 + 1 + 1e16 keeps them
    big = np.array([[1e16], [1.0], [1.0]])
    amount = lambda order: cell_spell_ref(big[order], [0, 3], [0, 1, 2], 0.0, np.zeros((1, 1)), None, 1, "amount")[0, 0, 0]
    assert amount([0, 1, 2]) == 1e16 and amount([1, 2, 0]) == 1e16 + 2.0


def test_planes_of_the_public_call():
    """planes=None / "month" / a callable, and the period that has no plane."""
    from climate_toolbox_amd.relative import resolve_planes
    assert resolve_planes([0], [2001, 2002, 2003], None).tolist() == [0, 0, 0]
    assert resolve_planes([2002, 2001], [2001, 2002], None).tolist() == [1, 0]
    with pytest.raises(ValueError, match="2003"):
        resolve_planes([2001, 2002], [2001, 2003], None)
    with pytest.raises(ValueError, match="plane per period"):
        resolve_planes([2001, 2002], [2001, 2002, 2003], None)
    months = np.arange(1, 13)
    got = resolve_planes(months, [200011, 200012, 200101, 200102], "month")
    assert got.tolist() == [10, 11, 0, 1] and got.dtype == np.int32
    with pytest.raises(ValueError, match="200107"):
        resolve_planes([1, 2, 12], [200101, 200107], "month")
    with pytest.raises(ValueError, match="year \\* 100"):
        resolve_planes(months, np.array(["a", "b"]), "month")
    assert resolve_planes(["cool", "warm"], [2001, 2002, 2003], lambda y: "warm" if y % 2 else "cool").tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="2002.*'mild'"):
        resolve_planes(["cool", "warm"], [2001, 2002], lambda y: "warm" if y % 2 else "mild")
    with pytest.raises(ValueError, match="planes must be"):
        resolve_planes([0], [1], "season")
    with pytest.raises(ValueError, match="planes must be"):
        resolve_planes([0], [1], 7)


def test_cell_thresholds_from_array_shapes():
    """2-D, 3-D and 4-D input, either grid order; defaults of labels and levels; what does not fit is ValueError."""
    from climate_toolbox_amd.relative import CellThresholds
    lat, lon = np.array([0.0, 0.5]), np.arange(4) * 0.5
    a = CellThresholds.from_array(np.zeros((2, 4)), lat, lon)
    assert a.values.shape == (1, 1, 2, 4) and (a.K, a.M) == (1, 1) and a.levels.tolist() == [0.0] and a.labels.tolist() == [0]
    assert a.shift == 0.0 and a.dims == ("lat", "lon")
    b = CellThresholds.from_array(np.zeros((3, 4, 2), dtype=np.float32), lat, lon, dims=("lon", "lat"), levels=[0.9, 0.95, 0.99], shift=-273.15)
    assert b.values.shape == (3, 1, 4, 2) and b.values.dtype == np.float32 and b.levels.tolist() == [0.9, 0.95, 0.99] and b.shift == -273.15
    c = CellThresholds.from_array(np.zeros((3, 12, 2, 4)), lat, lon, labels=np.arange(1, 13))
    assert c.values.shape == (3, 12, 2, 4) and c.labels.tolist() == list(range(1, 13)) and c.levels.tolist() == [0.0, 1.0, 2.0]
    assert CellThresholds.from_array(np.zeros((2, 4), dtype=np.int32), lat, lon).values.dtype == np.float64
    flat = CellThresholds(np.zeros((3, 2, 8)), 0.0, [1, 2, 3], ["a", "b"], lat, lon)
    assert (flat.K, flat.M) == (3, 2)
    for bad, kw in ((np.zeros(8), {}), (np.zeros((4, 2)), {}), (np.zeros((1, 1, 1, 2, 4)), {}), (np.zeros((2, 4)), {"dims": ("y", "x")}),
                    (np.zeros((2, 2, 4)), {"levels": [0.5]}), (np.zeros((1, 2, 2, 4)), {"labels": [1, 1]}),
                    (np.zeros((2, 4)), {"shift": float("nan")})):
        with pytest.raises(ValueError):
            CellThresholds.from_array(bad, lat, lon, **kw)


def _dataset():
    from climate_toolbox_amd import minixr
    tas = 280.0 + np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    return minixr.Dataset({"tas": (("time", "lat", "lon"), tas)},
                          coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})


def test_arguments_are_checked_before_any_device_work():
    """thresholds, stat, side, min_length (also for the two sums), planes, period, cells, leap_days: errors with no GPU in sight."""
    from climate_toolbox_amd import tas_relative_spell_aggregate
    from climate_toolbox_amd.relative import CellThresholds
    th = CellThresholds.from_array(np.zeros((2, 4)), np.array([0.0, 0.5]), np.arange(4) * 0.5)
    call = lambda **kw: tas_relative_spell_aggregate(kw.pop("ds", None), kw.pop("th", th), "popwt", "hierid", {}, **kw)
    with pytest.raises(TypeError, match="CellThresholds"):
        call(th=[30.0])
    for kw, match in ((dict(stat="mean"), "stat"), (dict(side="over"), "side"), (dict(min_length=0), "min_length"),
                      (dict(min_length=True), "min_length"), (dict(stat="longest", min_length=2), "longest"),
                      (dict(stat="amount", min_length=2), "amount"), (dict(stat="excess", min_length=6), "excess"),
                      (dict(stat="amount", th=CellThresholds.from_array(np.zeros((2, 4)), np.array([0.0, 0.5]), np.arange(4) * 0.5,
                                                                        shift=-273.15)), "final units"),
                      (dict(planes="year"), "planes"), (dict(period=None), "period="), (dict(cells="some"), "cells"),
                      (dict(leap_days="maybe"), "leap_days")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    two = CellThresholds.from_array(np.zeros((1, 2, 2, 4)), np.array([0.0, 0.5]), np.arange(4) * 0.5, labels=[1999, 2000])
    import pandas as pd
    df = pd.DataFrame({"lat": [0.0], "lon": [0.5], "areawt": [1.0], "popwt": [1.0], "hierid": ["a"]})
    with pytest.raises(ValueError, match="plane per period"):
        tas_relative_spell_aggregate(_dataset(), two, "popwt", "hierid", df)
