"""Sinusoid exposure bins, the part that needs no GPU: the exports of wagg_exposure_* (include/wagg.h), their bad-argument codes
and texts (all decided before any device call) in the order the grouped families share, the workspace rule, the argument checks
of snyder_exposure_aggregate that precede any device work, and the laws of the NumPy restatement (tests/exposure_ref.py) that
the GPU tests rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ref_numpy
from tests import exposure_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_exposure_reduce_f32", "wagg_exposure_reduce_f64", "wagg_exposure_work_bytes")
INF = float("inf")
P_ = C.c_void_p(0x1000)          # a device pointer no one may read


def _dbl(*v):
    return (C.c_double * len(v))(*v)


def test_exports_version_and_constants():
    """The three symbols are declared, bound and exported; the binding's constants are the header's; the version is 0.12.0."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, engine, seasons, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1200 and tuple(int(v) for v in pkg.__version__.split(".")) >= (0, 12, 0)
    assert int(re.search(r"#define WAGG_EXPOSURE_EDGES_MAX (\d+)", header).group(1)) == 65 == _lib.EXPOSURE_EDGES_MAX
    assert int(re.search(r"#define WAGG_EXPOSURE_GROUP (\d+)", header).group(1)) == _lib.EXPOSURE_GROUP
    assert 2 < _lib.EXPOSURE_GROUP < 15                        # (the GPU test's edge counts 3, G + 1, G + 2 and 17 are then distinct)
    assert callable(engine.exposure_reduce) and callable(seasons._exposure_totals)
    assert pkg.snyder_exposure_aggregate is transformations.snyder_exposure_aggregate
    assert "snyder_exposure_aggregate" in transformations.__all__


GOOD = dict(X=P_, X2=P_, T=10, n=8, ldx=8, rb=P_, rows=P_, P=2, n_rows=10, doy=P_, win=P_, offset=0.0, e=_dbl(*range(66)), n_edges=6, flags=0,
            out=P_, ldo=8, pstride=16, status=P_, work=None, work_bytes=0)


def _call(fn, **kw):
    a = dict(GOOD, **kw)
    return fn(a["X"], a["X2"], a["T"], a["n"], a["ldx"], a["rb"], a["rows"], a["P"], a["n_rows"], a["doy"], a["win"], a["offset"], a["e"],
              a["n_edges"], a["flags"], a["out"], a["ldo"], a["pstride"], a["status"], a["work"], a["work_bytes"], None)


@pytest.mark.parametrize("suffix", ["f32", "f64"])
def test_abi_bad_arguments_return_codes_and_texts(suffix):
    """Negative status + message, nothing thrown, nothing dereferenced; each requirement alone in its own words, and of two
    violated at once the earlier one speaks: sizes, flags, the family's own checks (n_edges, edges, offset, NaN, order), the
    doy / win pairing, the layout, and behind the empty return out and the two fields."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    fn = getattr(L, "wagg_exposure_reduce_" + suffix)
    nan = float("nan")

    def said(**kw):
        assert _call(fn, **kw) == -1, kw
        return L.wagg_last_error().decode()

    for n_edges in (1, 66, 0, -1):
        assert said(n_edges=n_edges) == "n_edges must be 2..65, got %d" % n_edges
    assert said(e=None) == "edges is NULL"
    for bad in (nan, INF, -INF):
        assert said(offset=bad) == "offset must be finite"
    assert said(e=_dbl(0.0, nan, 2.0), n_edges=3) == "edge 1 is NaN"
    assert said(e=_dbl(nan, 1.0), n_edges=2) == "edge 0 is NaN"
    assert said(e=_dbl(0.0, 2.0, 1.0), n_edges=3) == "edges must ascend strictly (edge 2 does not exceed edge 1)"
    assert said(e=_dbl(0.0, 1.0, 1.0), n_edges=3) == "edges must ascend strictly (edge 2 does not exceed edge 1)"
    assert said(e=_dbl(-INF, -INF, 1.0), n_edges=3) == "edges must ascend strictly (edge 1 does not exceed edge 0)"
    pairing = "doy_dev and win_dev go together: both given, or both NULL (no season)"
    assert said(doy=None) == pairing and said(win=None) == pairing
    flags_msg = "unknown flags 0x40 (an exposure total has no keep-NaN form)"
    assert said(flags=64) == flags_msg
    assert said(flags=_lib.PERIOD_KEEP_NAN) == "unknown flags 0x1 (an exposure total has no keep-NaN form)"
    sizes = "negative size (T=10, n=8, P=-1, n_rows=10)"
    for kw in ({"P": -1}, {"n": -3}, {"T": -1}, {"n_rows": -1}):
        assert "negative size" in said(**kw), kw
    assert "int32" in said(T=2 ** 31)
    layout = "ldx / ldo smaller than n (ldx=8, ldo=7, n=8)"
    assert said(ldo=7) == layout and "ldx / ldo smaller than n" in said(ldx=7)
    assert said(pstride=15) == "out_pstride smaller than P * ldo"
    assert said(out=None) == "NULL pointer (out_dev)"
    fields = "NULL pointer (tasmin_dev / tasmax_dev)"
    assert said(X=None) == fields and said(X2=None) == fields            # the second field is needed like the first
    assert _call(fn, work=C.c_void_p(0x1004), work_bytes=64) == -1 and _call(fn, work_bytes=-8) == -1
    # the order: sizes, flags, own checks, pairing, layout, out / fields
    bad_list = dict(e=_dbl(0.0, 10.0, 10.0, 30.0), n_edges=4)
    list_msg = "edges must ascend strictly (edge 2 does not exceed edge 1)"
    assert said(P=-1, flags=64) == sizes
    assert said(flags=64, n_edges=0) == flags_msg and said(flags=64, **bad_list) == flags_msg
    assert said(n_edges=0, win=None) == "n_edges must be 2..65, got 0"
    assert said(n_edges=0, e=None) == "n_edges must be 2..65, got 0"
    assert said(e=None, offset=nan) == "edges is NULL"
    assert said(offset=nan, **bad_list) == "offset must be finite"
    assert said(e=_dbl(0.0, 0.0, nan), n_edges=3) == "edges must ascend strictly (edge 1 does not exceed edge 0)"
    assert said(win=None, **bad_list) == list_msg and said(doy=None, **bad_list) == list_msg
    assert said(win=None, ldo=7) == pairing and said(doy=None, pstride=15) == pairing
    assert said(ldo=7, out=None) == layout and said(ldo=7, pstride=15) == layout
    assert said(pstride=15, status=None) == "out_pstride smaller than P * ldo"
    assert said(work_bytes=-8, status=None) == "work_dev must be 8-byte aligned, work_bytes >= 0"
    assert said(status=None, out=None) == "NULL pointer (status_dev / row_begin)"
    assert said(rows=None, out=None) == "NULL pointer (rows)"
    assert said(out=None, X=None) == "NULL pointer (out_dev)" and said(out=None, X2=None) == "NULL pointer (out_dev)"
    # nothing to do is not an error -- with or without a season, with open end bins -- and touches no device; an empty call
    # returns ahead of the out / field checks, but not ahead of the layout; one bin needs no plane stride
    assert _call(fn, P=0, out=None, X=None, X2=None) == 0 and _call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
    assert _call(fn, P=0, doy=None, win=None) == 0
    assert _call(fn, P=0, n_edges=65) == 0 and _call(fn, P=0, e=_dbl(-INF, 0.0, INF), n_edges=3) == 0
    assert _call(fn, n_edges=2, pstride=0, P=0, out=None) == 0
    assert said(P=0, ldo=7, out=None) == layout


def test_work_bytes_are_the_period_kernels_for_the_bins():
    """0 for non-positive arguments and for fewer than two edges; otherwise what wagg_period_reduce_work_bytes reports for
    n_edges - 1 planes as far as it takes planes (four), what the bins' and the ladder's rules give for as many planes beyond."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    wb, period, bins, ladder = L.wagg_exposure_work_bytes, L.wagg_period_reduce_work_bytes, L.wagg_bin_days_work_bytes, L.wagg_edd_ladder_work_bytes
    for args in ((0, 1, 10, 3), (63, 0, 10, 3), (63, 1, 0, 3), (63, 1, 10, 1), (63, 1, 10, 0), (-1, 1, 10, 3), (63, 1, 10, -2)):
        assert wb(*args) == 0, args
    some = 0
    for n in (1, 63, 256, 1025, 24378, 1036800):
        for P in (1, 2, 3, 4, 12, 70):
            for n_rows in (1, 9, 41, 70, 365, 3650):
                for planes in (1, 2, 3, 4):
                    assert wb(n, P, n_rows, planes + 1) == period(n, P, n_rows, planes), (n, P, n_rows, planes)
                for planes in (1, 4, 5, 8, 9, 17, 42, 64):
                    got = wb(n, P, n_rows, planes + 1)
                    assert got == bins(n, P, n_rows, planes + 1) == ladder(n, P, n_rows, planes), (n, P, n_rows, planes)
                    some += got > 0
    assert some > 10 and wb(1025, 1, 70, 2) > 0 and wb(1036800, 12, 365, 43) == 0


@pytest.mark.parametrize("bad", [[], (), [1.0], [1.0, 1.0], [2.0, 1.0], [0.0, float("nan")], [INF, 0.0], None, ["a", "b"], [[1.0, 2.0]]])
def test_edges_are_validated_before_any_device_work(bad):
    """Not even the dataset is looked at (None stands in for it)."""
    from climate_toolbox_amd import snyder_exposure_aggregate
    with pytest.raises(ValueError, match="edges"):
        snyder_exposure_aggregate(None, bad, "popwt", "hierid", {})


def test_arguments_are_checked_before_any_device_work():
    """period=None (with and without a season), cells outside its values, and fields of different units: refused with no GPU in
    sight, the units by the assertion snyder_edd makes."""
    from climate_toolbox_amd import minixr, snyder_exposure_aggregate
    edges = [0.0, 10.0, 20.0]
    with pytest.raises(ValueError, match="needs period=.*sum over days"):
        snyder_exposure_aggregate(None, edges, "popwt", "hierid", {}, period=None)
    with pytest.raises(ValueError, match="season= needs period="):
        snyder_exposure_aggregate(None, edges, "popwt", "hierid", {}, period=None, season=object())
    with pytest.raises(ValueError, match="cells must be"):
        snyder_exposure_aggregate(None, edges, "popwt", "hierid", {}, cells="some")
    lo = 10.0 + np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    ds = minixr.Dataset({"tasmin": (("time", "lat", "lon"), lo), "tasmax": (("time", "lat", "lon"), lo + 8.0)},
                        coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})
    ds["tasmin"].attrs["units"] = "C"
    ds["tasmax"].attrs["units"] = "K"
    with pytest.raises(AssertionError):
        snyder_exposure_aggregate(ds, edges, "popwt", "hierid", {})


# ---- the restatement's own laws, fp64 ---------------------------------------------------------------------------------------------
EDGES = [-INF] + [float(v) for v in np.arange(-5.0, 45.5, 2.5)] + [INF]


def _days(seed, T=60, n=23):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-10.0, 30.0, (T, n))
    hi = lo + rng.uniform(0.0, 18.0, (T, n))
    lo[3, 2] = hi[5, 4] = np.nan
    lo[7], hi[7] = 12.5, 12.5 + rng.uniform(0.0, 5.0, n)                 # tasmin on an edge
    hi[8] = 25.0                                                         # tasmax on an edge
    lo[8] = 25.0 - rng.uniform(0.0, 9.0, n)
    return lo, hi


def test_restated_fraction_at_hand_values():
    f = lambda lo, hi, e: float(ER.fraction_above(np.float64(lo), np.float64(hi), np.float64(e)))
    assert f(10, 20, 15) == 0.5 and f(10, 20, 10) == 1.0 and f(10, 20, 20) == 0.0 and f(10, 20, 5) == 1.0 and f(10, 20, 25) == 0.0
    assert abs(f(10, 20, 12.5) - 2.0 / 3.0) < 1e-15 and abs(f(10, 20, 17.5) - 1.0 / 3.0) < 1e-15
    assert f(np.nan, 20, -INF) == 0.0 and f(10, np.nan, 5) == 0.0 and f(10, 20, -INF) == 1.0 and f(10, 20, INF) == 0.0
    assert f(15, 15, 15) == 1.0 and f(15, 15, np.nextafter(15.0, 16.0)) == 0.0
    assert f(20, 10, 15) == 1.0 and f(20, 10, 20) == 1.0 and f(20, 10, 25) == 0.0       # inverted data: a step at tasmin
    assert 0.0 < f(10, np.nextafter(15.0, 16.0), 15) < 1e-7                            # tangency: small, positive, finite


def test_restated_bins_of_a_flat_day_are_the_day_counts():
    """tasmin == tasmax: bin k holds (x >= e_k) - (x >= e_k+1), exactly"""
    rng = np.random.default_rng(5)
    x = np.round(rng.uniform(-8.0, 44.0, (40, 17)) * 4) / 4              # (many values on the edges themselves)
    x[2, 3] = np.nan
    b = ER.day_bins(x, x, 0.0, EDGES)
    with np.errstate(invalid="ignore"):
        want = np.stack([(x >= EDGES[k]).astype(float) - (x >= EDGES[k + 1]).astype(float) for k in range(len(EDGES) - 1)])
    assert np.array_equal(b, want) and (b[:, 2, 3] == 0).all()


def test_restated_bins_sum_to_the_counted_days_and_are_not_negative():
    lo, hi = _days(11)
    T = lo.shape[0]
    rb, rows = np.array([0, 20, 20, 45, 61]), np.concatenate([np.arange(45), [44], np.arange(45, 60)])
    mask = (np.add.outer(np.arange(T), np.arange(lo.shape[1])) % 5 != 0).astype(float)
    for m in (None, mask):
        b = ER.exposure_bins(lo, hi, 0.0, EDGES, rb, rows, m)
        D = ER.counted_days(lo, hi, rb, rows, m)
        assert b.shape == (len(EDGES) - 1, 4, lo.shape[1]) and (b >= 0).all() and (b[:, 1] == 0).all()
        assert D.max() >= 16 and np.abs(b.sum(0) - D).max() <= 1e-12 * max(1.0, D.max())
        assert np.all(np.abs(b.sum(0) - D) <= 1e-12 * np.maximum(D, 1.0))


def test_restated_fraction_brackets_the_degree_day_differences():
    """A = -d EDD / de and A falls with e: per day (b - a) A(b) <= EDD(a) - EDD(b) <= (b - a) A(a), against the oracle's
    restatement of snyder_edd, to the rounding of its own expression (1e-12 on degree days of tens)."""
    lo, hi = _days(17)
    ok = ~(np.isnan(lo) | np.isnan(hi))
    ladder = [float(v) for v in np.arange(-12.0, 50.0, 1.25)]
    with np.errstate(invalid="ignore"):
        edd = [ref_numpy.snyder_edd_values(lo, hi, e) for e in ladder]
    A = [ER.fraction_above(lo, hi, np.float64(e)) for e in ladder]
    for k in range(len(ladder) - 1):
        a, b = ladder[k], ladder[k + 1]
        diff = (edd[k] - edd[k + 1])[ok]
        assert np.all((b - a) * A[k + 1][ok] - 1e-12 <= diff) and np.all(diff <= (b - a) * A[k][ok] + 1e-12), (a, b)
