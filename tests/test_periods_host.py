"""Period totals, the part that needs no GPU: which rows form which period (climate_toolbox_amd/periods.py: period_rows) and
the bad-argument codes of wagg_period_reduce_* (include/wagg.h), which are decided before any device call."""
import ctypes as C

import numpy as np
import pytest


def _lists(time, period):
    from climate_toolbox_amd.periods import period_rows
    labels, rb, rows = period_rows(time, period)
    return list(labels), [list(rows[rb[p]:rb[p + 1]]) for p in range(len(labels))]


def test_year_and_month_from_datetime64():
    t = np.arange("2003-12-30", "2004-03-02", dtype="datetime64[D]")          # 2 + 31 + 29 (a leap February) + 1 days
    labels, rows = _lists(t, "year")
    assert labels == [2003, 2004] and rows == [[0, 1], list(range(2, 63))]
    labels, rows = _lists(t, "month")
    assert labels == [200312, 200401, 200402, 200403]
    assert [len(r) for r in rows] == [2, 31, 29, 1]                           # 29 February is summed like any day
    assert rows[2] == list(range(33, 62))
    labels, rows = _lists(t.astype("datetime64[ns]"), "month")                # (any datetime64 unit)
    assert labels == [200312, 200401, 200402, 200403]


def test_year_and_month_from_yyyyddd():
    t = np.array([2001058, 2001059, 2001060, 2001365, 2002001, 2001001])
    labels, rows = _lists(t, "year")
    assert labels == [2001, 2002] and rows == [[0, 1, 2, 3, 5], [4]]
    labels, rows = _lists(t, "month")
    # day 59 = 28 February, day 60 = 1 March, day 365 = 31 December on the 365-day calendar
    assert labels == [200101, 200102, 200103, 200112, 200201]
    assert rows == [[5], [0, 1], [2], [3], [4]]
    from climate_toolbox_amd.periods import _year_month
    days = np.arange(1, 366) + 1999000
    month = _year_month(days)[1]
    assert list(np.bincount(month)[1:]) == [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    assert (np.diff(month) >= 0).all() and month[58] == 2 and month[59] == 3 and month[364] == 12


def test_explicit_labels_drop_rows_and_come_out_ascending():
    t = np.arange(7)
    labels, rows = _lists(t, [30, -1, 10, 30, 10, -7, 20])
    assert labels == [10, 20, 30] and rows == [[2, 4], [6], [0, 3]]           # ascending labels, rows in time order, negatives gone
    labels, rows = _lists(t, [30, None, 10, 30, 10, None, 20])
    assert labels == [10, 20, 30] and rows == [[2, 4], [6], [0, 3]]
    labels, rows = _lists(t, np.array(["b", "a", "b", "c", "a", "a", "b"]))
    assert labels == ["a", "b", "c"] and rows == [[1, 4, 5], [0, 2, 6], [3]]
    labels, rows = _lists(t, np.arange(7) % 3)                                # interleaved: non-contiguous rows
    assert rows == [[0, 3, 6], [1, 4], [2, 5]]
    labels, rows = _lists(t, [-1] * 7)
    assert labels == [] and rows == []


def test_csr_row_lists():
    from climate_toolbox_amd.periods import period_rows
    labels, rb, rows = period_rows(np.arange(6), [5, 5, -1, 2, 5, 2])
    assert rb.dtype == np.int64 and rows.dtype == np.int64
    assert list(labels) == [2, 5] and list(rb) == [0, 2, 5] and list(rows) == [3, 5, 0, 1, 4]


@pytest.mark.parametrize("time,period", [
    (np.arange(5), "week"), (np.arange(5), "years"), (np.arange(5), None), (np.arange(5), [1, 2]), (np.arange(5), np.zeros((5, 1))),
    (np.arange(5), 3), (np.arange(5), "year"), (np.arange(5.0) + 2001001, "year"), (np.array([2001000, 2001001]), "month"),
    (np.array([2001366]), "year"), (np.arange(3), np.array([True, False, True])),
])
def test_value_errors(time, period):
    from climate_toolbox_amd.periods import period_rows
    with pytest.raises(ValueError):
        period_rows(time, period)


def test_public_function_is_exported_and_refuses_bad_requests_before_any_device_work():
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import minixr, periods
    assert pkg.weighted_aggregate_grid_to_regions_periods is periods.weighted_aggregate_grid_to_regions_periods
    ds = minixr.Dataset({"v": (("lat", "lon"), np.zeros((2, 2)))}, coords={"lat": np.arange(2.0), "lon": np.arange(2.0)})
    with pytest.raises(ValueError, match="time"):
        pkg.weighted_aggregate_grid_to_regions_periods(ds, "v", "areawt", "reg", {})
    with pytest.raises(ValueError, match="_route"):
        periods._aggregate_periods(None, "v", "areawt", "reg", {}, "areawt", "year", np.arange(3), route="sideways")


def test_engine_checks_the_row_lists_on_the_host():
    from climate_toolbox_amd import engine
    for rb, rows, T in (([0, 2], [0, 5], 5), ([0, 2], [0, -1], 5), ([0, 3], [0, 1], 5), ([2, 1], [0, 1], 5), ([], [], 5)):
        with pytest.raises(ValueError):
            engine.period_lists(rb, rows, T)


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, nothing dereferenced: null pointers, P < 0, n_pow / n_thr out of range,
    ldx < n, unknown transform / flags (every check precedes the first device call)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)                      # never dereferenced by the checks below
    thr = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)

    def call(fn=L.wagg_period_reduce_f32, X=p, X2=None, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, transform=_lib.XF_NONE, offset=0.0,
             pow_first=1, n_pow=1, thresholds=None, n_thr=0, flags=0, out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, X2, T, n, ldx, rb, rows, P, n_rows, transform, offset, pow_first, n_pow, thresholds, n_thr, flags, out, ldo, pstride,
                  status, work, work_bytes, None)

    for fn in (L.wagg_period_reduce_f32, L.wagg_period_reduce_f64):
        assert call(fn, status=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, rb=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, rows=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, out=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, X=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, transform=_lib.XF_EDD, thresholds=thr, n_thr=2, X2=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, P=-1) == -1 and b"negative" in L.wagg_last_error()
        assert call(fn, n=-3) == -1 and call(fn, T=-1) == -1 and call(fn, n_rows=-1) == -1
        assert call(fn, T=2 ** 31) == -1 and b"int32" in L.wagg_last_error()
        assert call(fn, ldx=7) == -1 and b"ldx" in L.wagg_last_error()
        assert call(fn, ldo=7) == -1
        assert call(fn, transform=_lib.XF_POLY, n_pow=4, pstride=15) == -1 and b"out_pstride" in L.wagg_last_error()
        for n_pow in (0, 5, -1):
            assert call(fn, transform=_lib.XF_POLY, n_pow=n_pow) == -1 and b"n_pow" in L.wagg_last_error()
        assert call(fn, transform=_lib.XF_POLY, pow_first=0) == -1 and call(fn, transform=_lib.XF_POLY, pow_first=15, n_pow=3) == -1
        for n_thr in (0, 5):
            assert call(fn, transform=_lib.XF_EDD, X2=p, thresholds=thr, n_thr=n_thr) == -1 and b"n_thr" in L.wagg_last_error()
        assert call(fn, transform=_lib.XF_EDD, X2=p, thresholds=None, n_thr=2) == -1 and b"thresholds" in L.wagg_last_error()
        assert call(fn, transform=7) == -1 and b"transform" in L.wagg_last_error()
        assert call(fn, flags=64) == -1 and b"flags" in L.wagg_last_error()
        assert call(fn, work=C.c_void_p(0x1004), work_bytes=64) == -1 and call(fn, work_bytes=-8) == -1
        # nothing to do is not an error -- and still touches no device
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
    # the workspace a split needs: none for a grid that fills the device, none for lists too short to cut
    wb = L.wagg_period_reduce_work_bytes
    assert wb(1036800, 12, 365, 1) == 0 and wb(63, 70, 70, 1) == 0 and wb(0, 1, 10, 1) == 0 and wb(63, 0, 10, 1) == 0
    assert wb(24378, 1, 365, 1) >= 2 * 8 * 24378 and wb(24378, 1, 365, 4) == 4 * wb(24378, 1, 365, 1)


def test_the_three_work_bytes_entry_points_agree():
    """Period totals, season totals and degree-day ladders cut a period's row list into the same parts -- that is what makes an
    all-year season equal the period sum and a ladder plane equal the four-plane kernels' plane bit for bit -- so the workspace
    each asks for is the same number: no split, a split below the cap, the cap of 64, a split held down by the mean list length
    (n_rows / P / 8), and non-positive arguments."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    fns = (L.wagg_period_reduce_work_bytes, L.wagg_season_reduce_work_bytes, L.wagg_edd_ladder_work_bytes)
    splits = set()
    for n in (1, 63, 256, 1100, 300000, 0, -1):
        for P in (1, 3, 40, 0, -1):
            for n_rows in (0, 15, 16, 70, 5000, -1):
                for planes in (1, 4, 0, -1):
                    got = [int(f(n, P, n_rows, planes)) for f in fns]
                    assert got[0] == got[1] == got[2], (n, P, n_rows, planes, got)
                    if min(n, P, n_rows, planes) <= 0:
                        assert got[0] == 0
                    else:
                        assert got[0] % (8 * planes * P * n) == 0
                        splits.add(got[0] // (8 * planes * P * n))
    assert 0 in splits and 64 in splits and any(1 < s < 64 for s in splits) and 1 not in splits
    for f in fns:
        assert f(63, 1, 15, 1) == 0 and f(63, 1, 70, 1) == 8 * 8 * 63          # one block: 15 // 8 = 1 part, 70 // 8 = 8 parts
        assert f(63, 1, 5000, 1) == 64 * 8 * 63                                 # 625 parts by rows, 1024 wanted: the cap
        assert f(300000, 1, 5000, 4) == 4 * 8 * 4 * 300000                      # 293 blocks of 16-byte pieces: ceil(1024 / 293) = 4
        assert f(300000, 40, 5000, 1) == 0                                      # the grid fills the device
