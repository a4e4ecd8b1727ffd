"""Degree-day ladders, the part that needs no GPU: the exports of wagg_edd_ladder_* (include/wagg.h), their bad-argument codes
(all decided before any device call), the workspace rule, validate_edd_snyder_agriculture and the argument checks of
snyder_edd_aggregate that precede any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_edd_ladder_reduce_f32", "wagg_edd_ladder_reduce_f64", "wagg_edd_ladder_work_bytes")


def test_exports_and_constants():
    """The three symbols are declared, bound and exported; the binding's constants are the header's."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, engine, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert int(re.search(r"#define WAGG_EDD_LADDER_MAX (\d+)", header).group(1)) == _lib.EDD_LADDER_MAX == 64
    assert int(re.search(r"#define WAGG_EDD_LADDER_GROUP (\d+)", header).group(1)) == _lib.EDD_LADDER_GROUP
    assert 4 < _lib.EDD_LADDER_GROUP < 17                      # (the GPU test's ladder lengths G, G + 1 and 17 are then distinct)
    assert callable(engine.edd_ladder_reduce)
    assert pkg.snyder_edd_aggregate is transformations.snyder_edd_aggregate
    assert pkg.validate_edd_snyder_agriculture is transformations.validate_edd_snyder_agriculture
    assert {"snyder_edd_aggregate", "validate_edd_snyder_agriculture"} <= set(transformations.__all__)


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, nothing dereferenced (every pointer below is a number no one may read)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)
    thr = (C.c_double * 64)(*range(64))

    def call(fn, X=p, X2=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win=p, offset=0.0, thresholds=thr, n_thr=5, flags=0,
             out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, X2, T, n, ldx, rb, rows, P, n_rows, doy, win, offset, thresholds, n_thr, flags, out, ldo, pstride, status, work,
                  work_bytes, None)

    for fn in (L.wagg_edd_ladder_reduce_f32, L.wagg_edd_ladder_reduce_f64):
        for n_thr in (0, 65, -1):
            assert call(fn, n_thr=n_thr) == -1 and b"n_thr must be 1..64" in L.wagg_last_error()
        assert call(fn, thresholds=None) == -1 and b"thresholds is NULL" in L.wagg_last_error()
        assert call(fn, doy=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        assert call(fn, win=None) == -1 and b"doy_dev and win_dev go together" in L.wagg_last_error()
        assert call(fn, flags=64) == -1 and b"unknown flags" in L.wagg_last_error()
        assert call(fn, flags=_lib.PERIOD_KEEP_NAN) == -1 and b"unknown flags" in L.wagg_last_error()
        for kw in ({"P": -1}, {"n": -3}, {"T": -1}, {"n_rows": -1}):
            assert call(fn, **kw) == -1 and b"negative size" in L.wagg_last_error(), kw
        assert call(fn, T=2 ** 31) == -1 and b"int32" in L.wagg_last_error()
        assert call(fn, ldx=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, ldo=7) == -1 and b"ldx / ldo smaller than n" in L.wagg_last_error()
        assert call(fn, pstride=15) == -1 and b"out_pstride smaller than P * ldo" in L.wagg_last_error()
        assert call(fn, status=None) == -1 and b"NULL" in L.wagg_last_error()
        assert call(fn, rb=None) == -1 and call(fn, rows=None) == -1 and call(fn, out=None) == -1
        assert call(fn, X=None) == -1 and b"tasmin_dev" in L.wagg_last_error()
        assert call(fn, X2=None) == -1 and b"tasmax_dev" in L.wagg_last_error()
        assert call(fn, work=C.c_void_p(0x1004), work_bytes=64) == -1 and call(fn, work_bytes=-8) == -1
        # one plane needs no plane stride; nothing to do is not an error -- with or without a season, and touches no device
        assert call(fn, n_thr=1, pstride=0, P=0, out=None) == 0
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
        assert call(fn, P=0, doy=None, win=None) == 0


def test_work_bytes_follow_the_season_kernels_split():
    """0 for non-positive arguments; wagg_season_reduce_work_bytes up to four thresholds (the same parts: the bit-equality
    contract rests on it) and wagg_period_reduce_work_bytes; linear in n_thr beyond."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    wb, season, period = L.wagg_edd_ladder_work_bytes, L.wagg_season_reduce_work_bytes, L.wagg_period_reduce_work_bytes
    for args in ((0, 1, 10, 1), (63, 0, 10, 1), (63, 1, 0, 1), (63, 1, 10, 0), (-1, 1, 10, 1), (63, 1, 10, -2)):
        assert wb(*args) == 0, args
    some = 0
    for n in (1, 63, 256, 1100, 24378, 1036800):
        for P in (1, 2, 3, 12, 70):
            for n_rows in (1, 9, 70, 365, 3650):
                for k in (1, 2, 3, 4):
                    assert wb(n, P, n_rows, k) == season(n, P, n_rows, k) == period(n, P, n_rows, k), (n, P, n_rows, k)
                one = wb(n, P, n_rows, 1)
                some += one > 0
                for k in (5, 8, 9, 17, 41, 64):
                    assert wb(n, P, n_rows, k) == k * one, (n, P, n_rows, k)
    assert some > 10 and wb(1100, 1, 70, 1) > 0 and wb(1036800, 12, 365, 41) == 0


def _product(n_regions, ref_temps):
    from climate_toolbox_amd import minixr
    return minixr.Dataset({"edd": (("refTemp", "period", "hierid"), np.zeros((len(ref_temps), 1, n_regions), dtype=np.float32))},
                          coords={"refTemp": np.asarray(ref_temps, dtype=np.float64), "period": np.array([2001]),
                                  "hierid": np.array(["r%05d" % i for i in range(n_regions)])})


def test_validate_edd_snyder_agriculture():
    from climate_toolbox_amd import validate_edd_snyder_agriculture
    ladder = np.arange(0, 41)
    assert validate_edd_snyder_agriculture(_product(24378, ladder), ladder) is None
    assert validate_edd_snyder_agriculture(_product(24378, ladder), [8, 31.0]) is None
    with pytest.raises(AssertionError, match="hierid dims do not match 24378"):
        validate_edd_snyder_agriculture(_product(24377, ladder), ladder)
    with pytest.raises(AssertionError):
        validate_edd_snyder_agriculture(_product(24378, ladder), [8, 41])
    with pytest.raises(AssertionError):
        validate_edd_snyder_agriculture(_product(24378, ladder), [8.5])


@pytest.mark.parametrize("bad", [[], (), [10.0, 30.0, 10], [10.0, float("nan")], [float("inf")], None, ["a"], [[1.0, 2.0]]])
def test_thresholds_are_validated_before_any_device_work(bad):
    """Not even the dataset is looked at (None stands in for it)."""
    from climate_toolbox_amd import snyder_edd_aggregate
    with pytest.raises(ValueError, match="thresholds"):
        snyder_edd_aggregate(None, bad, "popwt", "hierid", {})


def test_season_needs_a_period():
    from climate_toolbox_amd import snyder_edd_aggregate
    with pytest.raises(ValueError, match="season= needs period="):
        snyder_edd_aggregate(None, [10.0, 30.0], "popwt", "hierid", {}, season=object())
