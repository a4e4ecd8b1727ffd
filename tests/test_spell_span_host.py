"""Spells that run across period boundaries, the part that needs no GPU: the NumPy restatement tests/spell_span_ref.py against
cases worked out by hand and against the laws that tie it to the truncating restatement tests/spell_ref.py; the exports of
wagg_spell_span_* and their bad-argument codes; the argument checks of ``span=`` that precede any device work; and which
symbol each value of ``span`` reaches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.spell_ref import WIN_INVERT, spell_ref
from tests.spell_span_ref import running_and_whole, spell_span_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_spell_span_f32", "wagg_spell_span_f64", "wagg_spell_span_work_bytes")
STATS = ("days", "events", "longest")


def _all(X, row_begin, rows, L, **kw):
    """(days, events, longest) of threshold 1.0 as nested lists [period][cell]"""
    X = np.asarray(X, dtype=np.float64)
    return tuple(spell_span_ref(X, row_begin, rows, 0.0, [1.0], L if stat != "longest" else 1, stat, **kw)[0].astype(int).tolist()
                 for stat in STATS)


# ---- the restatement against cases worked out by hand ------------------------------------------------------------------------------
def test_ref_the_issue_case_a_credit_over_several_lists_and_an_empty_one():
    """an all-hot cell, T = 10, lists [0..3], [4], [], [5..9], L = 6: the run reaches 6 on row 5, the first entry of the last
    list; its five earlier days lie in the lists before -- one in [4], none in the empty one, four in [0..3]"""
    X = np.ones((10, 1))
    rb, rows = [0, 4, 5, 5, 10], np.arange(10)
    days, events, longest = _all(X, rb, rows, 6)
    assert [d[0] for d in days] == [4, 1, 0, 5]
    assert [e[0] for e in events] == [0, 0, 0, 1]
    assert [m[0] for m in longest] == [4, 5, 0, 10]
    _, r, ell = running_and_whole(X, rb, rows, 0.0, [1.0])
    assert r[0, :, 0].tolist() == list(range(1, 11)) and ell[0, :, 0].tolist() == [10] * 10


def test_ref_a_spell_over_new_year():
    """20 December to 10 January, two years of 31 + 31 days (December, January as the two periods): 12 and 22"""
    X = np.zeros((62, 1))
    X[19:41] = 1
    assert _all(X, [0, 31, 62], np.arange(62), 6) == ([[12], [10]], [[1], [0]], [[12], [22]])
    # min_length 13: neither part reaches it alone; the run reaches it on 1 January, where it counts as one event
    assert _all(X, [0, 31, 62], np.arange(62), 13) == ([[12], [10]], [[0], [1]], [[12], [22]])
    assert _all(X, [0, 31, 62], np.arange(62), 23) == ([[0], [0]], [[0], [0]], [[12], [22]])


def test_ref_a_period_wholly_inside_one_spell_reports_at_least_its_own_length():
    X = np.ones((12, 1))
    X[0] = 0
    assert _all(X, [0, 4, 8, 12], np.arange(12), 1)[2] == [[3], [7], [11]]


def test_ref_a_row_gap_exactly_at_a_boundary_carries_nothing():
    """rows 0..3 | 5..8 (row 4 dropped between the lists): nothing joins; rows that repeat or descend at the boundary neither"""
    X = np.ones((10, 1))
    for rows in ([0, 1, 2, 3, 5, 6, 7, 8], [0, 1, 2, 3, 3, 4, 5, 6], [4, 5, 6, 7, 0, 1, 2, 3]):
        got = _all(X, [0, 4, 8], rows, 3)
        assert got == ([[4], [4]], [[1], [1]], [[4], [4]]), rows
        for stat, g in zip(STATS, got):
            want = spell_ref(X, [0, 4, 8], rows, 0.0, [1.0], 3 if stat != "longest" else 1, stat)[0].astype(int).tolist()
            assert g == want
    assert _all(X, [0, 4, 8], [0, 1, 2, 3, 4, 5, 6, 7], 3) == ([[4], [4]], [[1], [0]], [[4], [8]])
    # an out-of-range row as a list's last entry is cold, and the entry behind it joins nothing hot
    assert _all(X, [0, 4, 8], [0, 1, 2, 10, 4, 5, 6, 7], 3) == ([[3], [4]], [[1], [1]], [[3], [4]])
    assert _all(X, [0, 4, 8], [0, 1, 2, -1, 0, 1, 2, 3], 5) == ([[0], [0]], [[0], [0]], [[3], [4]])


def test_ref_nan_and_season_on_either_side_of_a_boundary():
    """NaN on the last day of a list, NaN on the first day of the next, a window that closes on the last day of a period"""
    X = np.ones((8, 4))
    X[3, 1] = np.nan
    X[4, 2] = np.nan
    rb, rows = [0, 4, 8], np.arange(8)
    assert _all(X, rb, rows, 1)[2] == [[4, 3, 4, 4], [8, 4, 3, 8]]
    doy = np.arange(10, 18)
    win = np.array([0 | 1023 << 10, 0 | 1023 << 10, 0 | 1023 << 10, 10 | 13 << 10])     # cell 3: in season on the first list only
    days, events, longest = _all(X, rb, rows, 5, doy=doy, windows=win)
    assert longest == [[4, 3, 4, 4], [8, 4, 3, 0]] and days == [[4, 0, 0, 0], [4, 0, 0, 0]] and events == [[0, 0, 0, 0], [1, 0, 0, 0]]
    inv = np.array([11 | 15 << 10 | WIN_INVERT])                                         # in season on days 10, 16, 17 only
    assert _all(X[:, :1], rb, rows, 1, doy=doy, windows=inv) == ([[1], [2]], [[1], [1]], [[1], [2]])


# ---- the laws ----------------------------------------------------------------------------------------------------------------------
def _random_case(seed, P=5, n=40):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 7, P)
    lengths[rng.integers(P)] = 0
    rows = np.arange(int(lengths.sum())) + np.cumsum(rng.uniform(size=int(lengths.sum())) < 0.08)     # a few dropped rows
    T = int(rows.max(initial=0)) + 2
    X = np.where(rng.uniform(size=(T, n)) < 0.8, 8.5, 1.5)
    X[rng.uniform(size=X.shape) < 0.03] = np.nan
    return X, np.concatenate([[0], np.cumsum(lengths)]), rows


@pytest.mark.parametrize("seed", range(6))
def test_sums_and_maxima_over_periods_equal_the_chain_as_one_list(seed):
    """sum_p DAYS, sum_p EVENTS and max_p LONGEST equal the truncating restatement on the chain taken as one list; LONGEST is
    never below the truncating value, DAYS summed never below the truncating sum"""
    X, rb, rows = _random_case(seed)
    one = [0, len(rows)]
    thr = [5.0, 0.0]
    for side in ("above", "below"):
        for L in (1, 2, 3, 6, len(rows) + 1):
            for stat in STATS:
                if stat == "longest" and L != 1:
                    continue
                got = spell_span_ref(X, rb, rows, 0.0, thr, L, stat, side)
                whole = spell_ref(X, one, rows, 0.0, thr, L, stat, side)[:, 0]
                cut = spell_ref(X, rb, rows, 0.0, thr, L, stat, side)
                if stat == "longest":
                    np.testing.assert_array_equal(got.max(axis=1), whole)
                    assert (got >= cut).all()
                else:
                    np.testing.assert_array_equal(got.sum(axis=1), whole)
                    assert stat == "events" or (got.sum(axis=1) >= cut.sum(axis=1)).all()      # (a cut run may count as two events)
    assert (spell_span_ref(X, rb, rows, 0.0, thr, 1, "longest") > spell_ref(X, rb, rows, 0.0, thr, 1, "longest")).any()


@pytest.mark.parametrize("seed", range(3))
def test_where_nothing_crosses_a_boundary_the_two_restatements_agree(seed):
    """a cold day in front of every boundary, and pooled lists whose neighbours never follow each other in time"""
    X, rb, rows = _random_case(seed + 10)
    Xc = X.copy()
    for p in range(1, len(rb) - 1):
        if rb[p] < len(rows):
            Xc[rows[rb[p]]] = 1.5                                                    # the first entry of every later list is cold
    for stat, L in (("days", 1), ("days", 3), ("events", 2), ("longest", 1)):
        np.testing.assert_array_equal(spell_span_ref(Xc, rb, rows, 0.0, [5.0], L, stat), spell_ref(Xc, rb, rows, 0.0, [5.0], L, stat))
    pooled_rows = np.array([0, 1, 2, 10, 11, 12, 3, 4, 5, 13, 14, 15])               # "months of all years": lists 0-2+10-12 | 3-5+13-15
    Xp = np.full((16, 3), 9.0)
    for stat, L in (("days", 4), ("events", 2), ("longest", 1)):
        np.testing.assert_array_equal(spell_span_ref(Xp, [0, 6, 12], pooled_rows, 0.0, [5.0], L, stat),
                                      spell_ref(Xp, [0, 6, 12], pooled_rows, 0.0, [5.0], L, stat))


# ---- the library and the binding ---------------------------------------------------------------------------------------------------
def test_exports_version_and_declarations():
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1800 and tuple(int(v) for v in pkg.__version__.split(".")) >= (0, 18, 0)
    for n in (0, 1, 1100, 1036800):
        for P in (0, 1, 12):
            for n_thr in (1, 8, 9, 64):
                assert L.wagg_spell_span_work_bytes(n, P, 3650, n_thr) == 0
    for word in ("CHAIN", "JOINS", "RUNNING LENGTH", "WHOLE LENGTH"):
        assert word in header, word


def test_abi_bad_arguments_return_codes():
    """wagg_spell_reduce_*'s checks, decided before any device call (every pointer below is a number no one may read)"""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)
    some = (C.c_double * 65)(*range(65))

    def call(fn, X=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win=p, offset=0.0, t=some, n_thr=5, L_=3, stat=0, below=0,
             flags=0, out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, T, n, ldx, rb, rows, P, n_rows, doy, win, offset, t, n_thr, L_, stat, below, flags, out, ldo, pstride, status, work,
                  work_bytes, None)

    for fn in (L.wagg_spell_span_f32, L.wagg_spell_span_f64):
        for n_thr in (0, 65, -1):
            assert call(fn, n_thr=n_thr) == -1 and b"n_thr must be 1..64" in L.wagg_last_error(), n_thr
        assert call(fn, t=None) == -1 and b"thresholds is NULL" in L.wagg_last_error()
        assert call(fn, t=(C.c_double * 2)(0.0, float("nan")), n_thr=2) == -1 and b"threshold 1 is NaN" in L.wagg_last_error()
        assert call(fn, t=(C.c_double * 1)(float("inf")), n_thr=1) == -1 and b"threshold 0 is infinite" in L.wagg_last_error()
        assert call(fn, offset=float("nan")) == -1 and b"offset must be finite" in L.wagg_last_error()
        for bad in (0, -1, 32768):
            assert call(fn, L_=bad) == -1 and b"min_length must be 1..32767" in L.wagg_last_error(), bad
        assert call(fn, stat=3, L_=1) == -1 and b"stat must be" in L.wagg_last_error()
        assert call(fn, stat=_lib.SPELL_LONGEST, L_=2) == -1 and b"WAGG_SPELL_LONGEST does not use min_length" in L.wagg_last_error()
        assert call(fn, below=2) == -1 and b"below must be 0 or 1" in L.wagg_last_error()
        assert call(fn, flags=64) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, doy=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        assert call(fn, P=-1) == -1 and b"negative size" in L.wagg_last_error()
        assert call(fn, ldo=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, pstride=15) == -1 and b"out_pstride smaller than P * ldo" in L.wagg_last_error()
        assert call(fn, status=None) == -1 and call(fn, out=None) == -1 and call(fn, X=None) == -1
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
        assert call(fn, P=0, L_=32767) == 0 and call(fn, P=0, work=C.c_void_p(0x1004), work_bytes=-8) == 0


def test_span_is_validated_before_any_device_work():
    """the public call and engine.spell_reduce: anything but "period" / "record" is ValueError, with no dataset and no tensor"""
    from climate_toolbox_amd import engine, tas_spell_aggregate
    for bad in ("year", "Record", None, True, 1, ""):
        with pytest.raises(ValueError, match="span must be"):
            tas_spell_aggregate(None, [1.0], "popwt", "hierid", {}, span=bad)
        with pytest.raises(ValueError, match="span must be"):
            engine.spell_reduce(np.zeros((3, 4), dtype=np.float32), [0, 3], [0, 1, 2], 0.0, [1.0], span=bad)
    for span in ("period", "record"):                                  # the other checks are reached, in their old order
        with pytest.raises(ValueError, match="thresholds"):
            tas_spell_aggregate(None, [], "popwt", "hierid", {}, span=span)
        with pytest.raises(ValueError, match="longest"):
            tas_spell_aggregate(None, [1.0], "popwt", "hierid", {}, stat="longest", min_length=2, span=span)
        with pytest.raises(ValueError, match="needs period="):
            tas_spell_aggregate(None, [1.0], "popwt", "hierid", {}, period=None, span=span)
        with pytest.raises((TypeError, ValueError)):
            engine.spell_reduce(np.zeros((3, 4), dtype=np.float32), [0, 3], [0, 1, 2], 0.0, [1.0], span=span)


def test_each_span_reaches_its_own_symbol(monkeypatch):
    """span="period" (and no span at all) still calls wagg_spell_reduce, "record" wagg_spell_span, with one argument list"""
    from climate_toolbox_amd import engine
    seen = []
    monkeypatch.setattr(engine, "_check_X", lambda X, layout: X)
    monkeypatch.setattr(engine, "_grouped_reduce", lambda name, fields, *a: seen.append((name, a[5:8])) or (None, None))
    X = np.zeros((3, 4), dtype=np.float32)
    engine.spell_reduce(X, [0, 3], [0, 1, 2], 0.0, [1.0, 2.0], min_length=2)
    engine.spell_reduce(X, [0, 3], [0, 1, 2], 0.0, [1.0, 2.0], min_length=2, span="period")
    engine.spell_reduce(X, [0, 3], [0, 1, 2], 0.0, [1.0, 2.0], min_length=2, span="record")
    assert [s[0] for s in seen] == ["wagg_spell_reduce", "wagg_spell_reduce", "wagg_spell_span"]
    mids = [s[1][1][1:] for s in seen]                                 # (n_thr, min_length, stat, below) behind the pointer
    assert mids[0] == mids[1] == mids[2] == (2, 2, 0, 0) and all(s[1][0] == 0.0 and s[1][2] == 2 for s in seen)
