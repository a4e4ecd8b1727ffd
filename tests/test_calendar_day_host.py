"""Calendar-day thresholds, the part that needs no GPU: relative.calendar_day_rows and relative.resolve_row_planes, the argument
errors relative.cell_spell_reduce raises before it touches a device, the exports of wagg_row_cell_spells_*, and the NumPy
restatement tests/cell_spell_rows_ref.py against tests/cell_spell_ref.py where the two definitions meet."""
import os
import re

import numpy as np
import pytest

from tests.cell_spell_ref import cell_spell_ref
from tests.cell_spell_rows_ref import cell_spell_rows_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (not wagg_cell_spells_rows_*: tests/test_cell_spell_host.py holds the wagg_cell_* names of the binding list to the by-period pair)
NAMES = ("wagg_row_cell_spells_f32", "wagg_row_cell_spells_f64")


def _labels(t):
    t = np.asarray(t).astype("datetime64[D]")
    m = t.astype("datetime64[M]")
    return (m.astype(int) % 12 + 1) * 100 + (t - m.astype("datetime64[D]")).astype(int) + 1


def test_exports_and_version():
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
        assert "plane_of_row_dev" in header[header.index(name):header.index(name) + 700]
    assert L.wagg_version() >= 1700 and tuple(int(v) for v in pkg.__version__.split(".")) >= (0, 17, 0)
    assert os.path.exists(os.path.join(ROOT, "climate_toolbox_amd", "csrc", "wagg_cell_spells_rows.hip"))


def test_calendar_day_rows_on_datetimes_with_a_leap_day():
    from climate_toolbox_amd.periods import period_rows
    from climate_toolbox_amd.relative import calendar_day_rows
    t = np.arange("2003-01-01", "2005-01-01", dtype="datetime64[D]")              # 365 + 366 days
    T = len(t)
    lab = _labels(t)
    labels, rb, rows = calendar_day_rows(t, window=5)
    assert len(labels) == 366 and labels.tolist() == sorted(set(lab.tolist())) and 229 in labels.tolist()
    assert rb[0] == 0 and rb[-1] == len(rows) and rows.dtype == np.int64
    for c in (101, 102, 103, 228, 229, 301, 704, 1230, 1231):
        k = labels.tolist().index(c)
        want = np.concatenate([np.arange(max(tt - 2, 0), min(tt + 2, T - 1) + 1) for tt in np.flatnonzero(lab == c)])
        assert rows[rb[k]:rb[k + 1]].tolist() == want.tolist(), c
    n = np.diff(rb)
    ix = {c: k for k, c in enumerate(labels.tolist())}
    assert n[ix[101]] == 3 + 5 and n[ix[102]] == 4 + 5 and n[ix[1231]] == 5 + 3 and n[ix[1230]] == 5 + 4 and n[ix[229]] == 5
    assert n[ix[704]] == 10 and set(np.delete(n, [ix[c] for c in (101, 102, 1230, 1231, 229)]).tolist()) == {10}
    # window = 1: period_rows with the same labels
    for a, b in zip(calendar_day_rows(t, window=1), period_rows(t, lab)):
        assert np.array_equal(a, b)


def test_calendar_day_rows_on_yyyyddd_and_list_lengths():
    from climate_toolbox_amd.relative import calendar_day_rows
    y = np.concatenate([2001 * 1000 + np.arange(1, 366), 2002 * 1000 + np.arange(1, 366)])
    labels, rb, rows = calendar_day_rows(y, window=3)
    assert len(labels) == 365 and labels[0] == 101 and labels[58] == 228 and labels[59] == 301 and labels[-1] == 1231
    assert rows[rb[0]:rb[1]].tolist() == [0, 1, 364, 365, 366] and rows[rb[364]:rb[365]].tolist() == [363, 364, 365, 728, 729]
    assert rows[rb[59]:rb[60]].tolist() == [58, 59, 60, 423, 424, 425]
    y30 = np.concatenate([k * 1000 + np.arange(1, 366) for k in range(1981, 2011)])
    labels, rb, rows = calendar_day_rows(y30, window=5)
    n = np.diff(rb)
    assert len(labels) == 365 and n[:2].tolist() == [148, 149] and n[-2:].tolist() == [149, 148] and (n[2:-2] == 150).all()
    labels, rb, rows = calendar_day_rows(y30, window=31)
    assert np.diff(rb).max() == 930


def test_calendar_day_rows_errors():
    from climate_toolbox_amd.relative import calendar_day_rows
    t = np.arange("2003-01-01", "2004-01-01", dtype="datetime64[D]")
    for w in (0, 2, 4, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="odd integer"):
            calendar_day_rows(t, window=w)
    with pytest.raises(ValueError, match=r"time\[40\].*gap"):
        calendar_day_rows(np.delete(t, 40))
    with pytest.raises(ValueError, match=r"time\[41\].*repeat"):
        calendar_day_rows(np.insert(t, 40, t[40]))
    y = np.concatenate([2001 * 1000 + np.arange(1, 366), 2002 * 1000 + np.arange(2, 366)])
    with pytest.raises(ValueError, match=r"time\[365\]"):
        calendar_day_rows(y)
    with pytest.raises(ValueError, match="YYYYDDD"):
        calendar_day_rows(np.array([2001366, 2002001]))
    with pytest.raises(ValueError, match="dtype"):
        calendar_day_rows(np.arange(10.0))
    # a record whose 29 February was removed is consecutive on its own calendar
    t4 = np.arange("2004-01-01", "2005-01-01", dtype="datetime64[D]")
    labels, rb, rows = calendar_day_rows(t4[_labels(t4) != 229], window=3)
    assert len(labels) == 365 and rows[rb[58]:rb[59]].tolist() == [57, 58, 59]     # 27, 28 February, 1 March


def test_resolve_row_planes():
    from climate_toolbox_amd.relative import calendar_day_rows, resolve_row_planes
    t = np.arange("2004-01-01", "2005-01-01", dtype="datetime64[D]")
    labels, _, _ = calendar_day_rows(t, window=1)
    got = resolve_row_planes(labels, t)
    assert got.dtype == np.int32 and got.tolist() == list(range(366))
    shuffled = labels[::-1].copy()
    assert resolve_row_planes(shuffled, t).tolist() == list(range(365, -1, -1))
    y = 2001 * 1000 + np.arange(1, 366)
    assert resolve_row_planes(labels, y).tolist() == [k for k in range(366) if k != 59]
    no_leap = labels[labels != 229]
    with pytest.raises(ValueError, match="2004-02-29"):
        resolve_row_planes(no_leap, t)
    listed = np.flatnonzero(_labels(t) != 229)
    got = resolve_row_planes(no_leap, t, rows=listed)                               # a day no period lists needs no plane
    assert got[59] == -1 and (got[listed] >= 0).all()
    with pytest.raises(ValueError, match="month \\* 100 \\+ day"):
        resolve_row_planes(np.array(["a", "b"]), t)


def test_cell_spell_reduce_refuses_both_maps_before_any_device_use():
    from climate_toolbox_amd.relative import cell_spell_reduce
    with pytest.raises(ValueError, match="exclude each other"):
        cell_spell_reduce(None, [0, 1], [0], 0.0, None, plane_of_period=[0], plane_of_row=[0])


def test_the_restatement_meets_the_by_period_one():
    """plane_of_row = the plane of the row's period: the two NumPy restatements agree wherever every cell has a counted entry;
    a NaN threshold on a day the cell is not counted leaves 0 here and NaN there."""
    rng = np.random.default_rng(3)
    T, n, K, M = 23, 7, 3, 2
    rb, rows = np.array([0, 9, 17, 17]), np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17])
    X = rng.uniform(0, 10, (T, n))
    X[6, 2] = np.nan
    thr = rng.uniform(2, 8, (K, M, n))
    pper = [1, 0, 1]
    prow = np.asarray(pper)[np.repeat([0, 1, 2], [10, 8, 5])]
    for stat, L in (("days", 1), ("days", 3), ("events", 2), ("longest", 1), ("amount", 1), ("excess", 1)):
        for side in ("above", "below"):
            a = cell_spell_ref(X, rb, rows, -1.5, thr, pper, L, stat, side)
            b = cell_spell_rows_ref(X, rb, rows, -1.5, thr, prow, L, stat, side)
            assert np.array_equal(a, b), (stat, side)
    thr[1, 1, 4] = np.nan
    a = cell_spell_ref(X, rb, rows, 0.0, thr, pper)
    b = cell_spell_rows_ref(X, rb, rows, 0.0, thr, prow)
    assert np.isnan(a[1, [0, 2], 4]).all() and np.isnan(b[1, [0, 2], 4]).tolist() == [True, False] and b[1, 2, 4] == 0   # (plane 1: periods 0, 2)
    bad = prow.copy()
    bad[12] = 2
    assert np.isnan(cell_spell_rows_ref(X, rb, rows, 0.0, thr, bad)[:, 1]).all()
    bad = prow.copy()
    bad[4] = bad[20] = 9                                                            # rows no list names
    assert np.array_equal(cell_spell_rows_ref(X, rb, rows, 0.0, thr, bad), b, equal_nan=True)
