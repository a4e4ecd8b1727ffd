"""The order of the argument checks of the three grouped row-list entry points (wagg_edd_ladder_reduce_*, wagg_bin_days_reduce_*,
wagg_hinge_reduce_*), which share one host sequence (csrc/wagg_rowlist.h, grouped_reduce): calls that violate two requirements
at once must report the one that has always come first, in the words it has always had.  Every check runs before any device
work, so none of this needs a GPU; the expected texts were recorded from the three separate host functions that preceded the
shared one."""
import ctypes as C

import pytest

P_ = C.c_void_p(0x1000)          # a device pointer no one may read


def _dbl(*v):
    return (C.c_double * len(v))(*v)


GOOD = dict(T=10, n=8, ldx=8, rb=P_, rows=P_, P=2, n_rows=10, doy=P_, win=P_, offset=0.0, flags=0, out=P_, ldo=8, pstride=16, status=P_,
            work=None, work_bytes=0)


def _ladder(L, suffix, X=P_, X2=P_, params=_dbl(10.0, 20.0, 30.0), count=3, **kw):
    a = dict(GOOD, **kw)
    return getattr(L, "wagg_edd_ladder_reduce_" + suffix)(
        X, X2, a["T"], a["n"], a["ldx"], a["rb"], a["rows"], a["P"], a["n_rows"], a["doy"], a["win"], a["offset"], params, count, a["flags"],
        a["out"], a["ldo"], a["pstride"], a["status"], a["work"], a["work_bytes"], None)


def _bins(L, suffix, X=P_, X2=None, params=_dbl(0.0, 10.0, 20.0, 30.0), count=4, **kw):
    a = dict(GOOD, **kw)
    return getattr(L, "wagg_bin_days_reduce_" + suffix)(
        X, a["T"], a["n"], a["ldx"], a["rb"], a["rows"], a["P"], a["n_rows"], a["doy"], a["win"], a["offset"], params, count, a["flags"],
        a["out"], a["ldo"], a["pstride"], a["status"], a["work"], a["work_bytes"], None)


def _hinge(L, suffix, X=P_, X2=None, params=_dbl(10.0, 20.0, 30.0), count=3, power=1, **kw):
    a = dict(GOOD, **kw)
    return getattr(L, "wagg_hinge_reduce_" + suffix)(
        X, a["T"], a["n"], a["ldx"], a["rb"], a["rows"], a["P"], a["n_rows"], a["doy"], a["win"], a["offset"], params, count, power, 0,
        None, None, None, a["flags"], a["out"], a["ldo"], a["pstride"], a["status"], a["work"], a["work_bytes"], None)


PAIRING = "doy_dev and win_dev go together: both given, or both NULL (no season)"
LAYOUT = "ldx / ldo smaller than n (ldx=8, ldo=7, n=8)"
# per family: the call, a bad parameter list and its message, and the family's own words in the shared checks
FAMILIES = {
    "ladder": (_ladder, dict(params=None), "thresholds is NULL", "n_thr must be 1..64, got 0",
               "unknown flags 0x40 (a degree-day ladder has no keep-NaN form)", "NULL pointer (tasmin_dev / tasmax_dev)"),
    "bins": (_bins, dict(params=_dbl(0.0, 10.0, 10.0, 30.0)), "edges must ascend strictly (edge 2 does not exceed edge 1)",
             "n_edges must be 2..65, got 0", "unknown flags 0x40 (a bin count has no keep-NaN form)", "NULL pointer (X_dev)"),
    "hinge": (_hinge, dict(params=_dbl(10.0, float("inf"), 30.0)), "knot 1 is not finite", "n_knots must be 1..64, got 0",
              "unknown flags 0x40 (a hinge total has no keep-NaN form)", "NULL pointer (X_dev)"),
}


@pytest.mark.parametrize("suffix", ["f32", "f64"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_first_violated_requirement_is_reported(family, suffix):
    from climate_toolbox_amd import _lib
    L = _lib.load()
    call, bad_list, list_msg, count_msg, flags_msg, field_msg = FAMILIES[family]

    def said(**kw):
        assert call(L, suffix, **kw) == -1, kw
        return L.wagg_last_error().decode()

    # each requirement alone says what it says ...
    assert said(P=-1) == "negative size (T=10, n=8, P=-1, n_rows=10)"
    assert said(flags=64) == flags_msg
    assert said(count=0) == count_msg
    assert said(**bad_list) == list_msg
    assert said(win=None) == PAIRING and said(doy=None) == PAIRING
    assert said(ldo=7) == LAYOUT
    assert said(pstride=15) == "out_pstride smaller than P * ldo"
    assert said(out=None) == "NULL pointer (out_dev)"
    assert said(X=None) == field_msg
    # ... and of two violated at once the earlier one speaks: sizes, flags, the family's parameter list (its count first), the
    # doy / win pairing, the layout (strides, workspace, status and lists), and behind the empty return out and the field(s)
    assert said(P=-1, flags=64) == "negative size (T=10, n=8, P=-1, n_rows=10)"
    assert said(flags=64, count=0) == flags_msg
    assert said(flags=64, **bad_list) == flags_msg
    assert said(count=0, win=None) == count_msg
    assert said(win=None, **bad_list) == list_msg
    assert said(doy=None, **bad_list) == list_msg
    assert said(win=None, ldo=7) == PAIRING
    assert said(doy=None, pstride=15) == PAIRING
    assert said(ldo=7, out=None) == LAYOUT
    assert said(ldo=7, pstride=15) == LAYOUT
    assert said(pstride=15, status=None) == "out_pstride smaller than P * ldo"
    assert said(work_bytes=-8, status=None) == "work_dev must be 8-byte aligned, work_bytes >= 0"
    assert said(status=None, out=None) == "NULL pointer (status_dev / row_begin)"
    assert said(rows=None, out=None) == "NULL pointer (rows)"
    assert said(out=None, X=None) == "NULL pointer (out_dev)"
    # an empty call returns ahead of the out / field checks, but not ahead of the layout
    assert call(L, suffix, P=0, out=None, X=None) == 0
    assert said(P=0, ldo=7, out=None) == "ldx / ldo smaller than n (ldx=8, ldo=7, n=8)"


def test_only_the_ladder_needs_a_second_field():
    from climate_toolbox_amd import _lib
    L = _lib.load()
    for suffix in ("f32", "f64"):
        assert _ladder(L, suffix, X2=None) == -1 and L.wagg_last_error().decode() == "NULL pointer (tasmin_dev / tasmax_dev)"
        assert _ladder(L, suffix, X2=None, out=None) == -1 and L.wagg_last_error().decode() == "NULL pointer (out_dev)"
