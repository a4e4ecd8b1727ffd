"""Period quantiles, the part that needs no GPU: the exports of wagg_quantile_select_* (include/wagg.h) and their constants, every
bad-argument code with its message (all decided before any device call), the naming rule that keeps the two symbols out of the
wagg_*_reduce_* pattern (the row-list layout table names them by their own symbol), the binding's and the public call's argument
checks that precede any device work, the NumPy restatement tests/quantile_ref.py against np.quantile / np.sort, and the long shape
of that module, which tests/test_gpu_quantile.py runs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import quantile_ref as QR
from tests.quantile_ref import quantile_ref
from tests.rolling_ref import WIN_INVERT, WIN_NULL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wagg_quantile_select_f32", "wagg_quantile_select_f64")


def test_exports_version_and_constants():
    """The two symbols are declared, bound and exported; the binding's constants are the header's; the version is 0.15.0."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, engine, seasons, transformations
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert L.wagg_version() >= 1500 and tuple(int(v) for v in pkg.__version__.split(".")) >= (0, 15, 0)
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))
    assert define("WAGG_QUANT_MAX") == _lib.QUANT_MAX == 16
    assert define("WAGG_QUANT_ROWS_MAX") == _lib.QUANT_ROWS_MAX == 1024
    assert (define("WAGG_QUANT_LINEAR"), define("WAGG_QUANT_LOWER"), define("WAGG_QUANT_HIGHER")) == (
        _lib.QUANT_LINEAR, _lib.QUANT_LOWER, _lib.QUANT_HIGHER) == (0, 1, 2)
    assert callable(engine.quantile_select) and callable(seasons._quantile_totals)
    assert pkg.tas_quantile_aggregate is transformations.tas_quantile_aggregate and "tas_quantile_aggregate" in transformations.__all__


def test_names_stay_out_of_the_reduce_pattern_and_there_is_no_workspace_export():
    """No export of this family matches wagg_(\\w+)_reduce_(f32|f64) (tests/rowlist_layout.py has it under its own symbol,
    ``entry="wagg_quantile_select"``, with no ``work_bytes``), and there is no wagg_quantile*_work_bytes: a list is never split."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    ours = [name for name in _lib.EXPORTS if "quantile" in name]
    assert sorted(ours) == sorted(NAMES)
    for name in ours:
        assert not re.fullmatch(r"wagg_(\w+)_reduce_(f32|f64)", name) and not name.endswith("_work_bytes"), name
    header = open(os.path.join(ROOT, "include", "wagg.h")).read()
    assert not re.search(r"\bwagg_quantile\w*_(reduce_f32|reduce_f64|work_bytes)\s*\(", header)
    for name in ("wagg_quantile_work_bytes", "wagg_quantile_select_work_bytes", "wagg_quantile_reduce_f32", "wagg_quantile_reduce_f64"):
        assert not hasattr(L, name), name


def test_binding_takes_stream_last_and_says_what_still_blocks():
    """engine.quantile_select has ``stream=None`` behind the parameters it had, and a probe in tests/test_gpu_stream_order.py that
    passes max_rows; its docstring still says that max_rows=None on device lists blocks, and now on which stream."""
    from climate_toolbox_amd import engine
    from tests import test_gpu_stream_order as probes
    params = inspect.signature(engine.quantile_select).parameters
    assert list(params) == ["X", "row_begin", "rows", "offset", "q", "method", "max_rows", "doy", "windows", "checked", "out", "status",
                            "stream"]
    assert params["stream"].default is None
    doc = " ".join(engine.quantile_select.__doc__.split())
    assert "NO ``stream=``" not in doc and "``stream=``" in doc
    assert "``row_begin.diff().max()``" in doc and "blocks" in doc and "CURRENT stream" in doc and "passes ``max_rows``" in doc
    assert "quantile_select" in probes.ROWLIST and "quantile_select" in probes.PROBES and "quantile_select" not in probes.EXEMPT
    src = inspect.getsource(probes)
    assert re.search(r"e\.quantile_select\([^\n]*max_rows=9, checked=True, stream=s", src)


def test_abi_bad_arguments_return_codes():
    """Negative status + message, nothing thrown, nothing dereferenced (every device pointer below is a number no one may read)."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)

    def lv(*v):
        return (C.c_double * len(v))(*v)

    some = lv(0.0, 0.05, 1.0 / 3.0, 0.5, 0.9, 0.95, 1.0, 0.5, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7, 0.8, 0.99)

    def call(fn, X=p, T=10, n=8, ldx=8, rb=p, rows=p, P=2, n_rows=10, doy=p, win_=p, offset=0.0, q=some, n_q=4, method=0, max_rows=10,
             flags=0, out=p, ldo=8, pstride=16, status=p, work=None, work_bytes=0):
        return fn(X, T, n, ldx, rb, rows, P, n_rows, doy, win_, offset, q, n_q, method, max_rows, flags, out, ldo, pstride, status, work,
                  work_bytes, None)

    inf, nan = float("inf"), float("nan")
    for fn in (L.wagg_quantile_select_f32, L.wagg_quantile_select_f64):
        for n_q in (0, 17, -1):
            assert call(fn, n_q=n_q) == -1 and b"n_q must be 1..16" in L.wagg_last_error(), n_q
        assert call(fn, q=None) == -1 and b"q is NULL" in L.wagg_last_error()
        assert call(fn, q=lv(0.5, -0.1, 0.2), n_q=3) == -1 and b"quantile 1 must lie in [0, 1]" in L.wagg_last_error()
        assert call(fn, q=lv(1.5), n_q=1) == -1 and b"quantile 0 must lie in [0, 1]" in L.wagg_last_error()
        assert call(fn, q=lv(0.5, 0.25, nan), n_q=3) == -1 and b"quantile 2 must lie in [0, 1]" in L.wagg_last_error()
        for bad in (3, -1, 17):
            assert call(fn, method=bad) == -1 and b"method must be" in L.wagg_last_error(), bad
        for bad in (0, 1025, -5):
            assert call(fn, max_rows=bad) == -1 and b"max_rows must be 1..1024" in L.wagg_last_error(), bad
        assert call(fn, offset=nan) == -1 and call(fn, offset=inf) == -1 and b"offset must be finite" in L.wagg_last_error()
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
        # nothing to do is not an error -- with or without a season, every method, unsorted levels with duplicates, the limits
        # themselves -- and touches no device; one level needs no plane stride; the workspace arguments are not looked at
        assert call(fn, P=0, out=None, X=None) == 0 and call(fn, n=0, ldx=0, ldo=0, out=None, X=None) == 0
        assert call(fn, P=0, doy=None, win_=None) == 0
        assert call(fn, P=0, n_q=16) == 0 and call(fn, P=0, q=lv(1.0, 0.0, 1.0), n_q=3) == 0
        assert call(fn, P=0, method=_lib.QUANT_LOWER, offset=-273.15) == 0 and call(fn, P=0, method=_lib.QUANT_HIGHER) == 0
        assert call(fn, P=0, max_rows=1) == 0 and call(fn, P=0, max_rows=1024) == 0
        assert call(fn, n_q=1, pstride=0, P=0, out=None) == 0
        assert call(fn, P=0, work=C.c_void_p(0x1004), work_bytes=-8) == 0


@pytest.mark.parametrize("bad", [[], (), [-0.1], [1.5], [float("nan")], [True], [np.True_], ["0.5"], [None], [0.5, 2], [float("inf")], None])
def test_levels_are_validated_before_any_device_work(bad):
    """-0.1, 1.5, NaN, True, an empty list ...: not even the dataset is looked at (None stands in for it)."""
    from climate_toolbox_amd import tas_quantile_aggregate
    with pytest.raises(ValueError, match="q must be"):
        tas_quantile_aggregate(None, bad, "popwt", "hierid", {})


def test_arguments_are_checked_before_any_device_work():
    """method; period=None, cells, leap_days; a power variable; a period of more than 1024 days: ValueError, with no GPU in sight."""
    from climate_toolbox_amd import minixr, tas_quantile_aggregate
    from climate_toolbox_amd.transformations import tas_poly
    q = [0.5, 0.05, 1, 0, np.float32(0.25), 0.5]
    for bad in ("nearest", "midpoint", None, 0):
        with pytest.raises(ValueError, match="method must be"):
            tas_quantile_aggregate(None, q, "popwt", "hierid", {}, method=bad)
    with pytest.raises(ValueError, match="needs period="):
        tas_quantile_aggregate(None, q, "popwt", "hierid", {}, period=None)
    with pytest.raises(ValueError, match="season= needs period="):
        tas_quantile_aggregate(None, q, "popwt", "hierid", {}, period=None, season=object())
    with pytest.raises(ValueError, match="cells must be"):
        tas_quantile_aggregate(None, q, "popwt", "hierid", {}, cells="some")
    with pytest.raises(ValueError, match="leap_days"):
        tas_quantile_aggregate(None, q, "popwt", "hierid", {}, leap_days="maybe")
    tas = 280.0 + np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    ds = minixr.Dataset({"tas": (("time", "lat", "lon"), tas)},
                        coords={"time": np.datetime64("2001-01-01") + np.arange(3), "lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5})
    with pytest.raises(ValueError, match="plain"):
        tas_quantile_aggregate(tas_poly(ds, 2, "tas-poly-2"), q, "popwt", "hierid", {}, tas="tas-poly-2")
    with pytest.raises(ValueError, match="time"):
        tas_quantile_aggregate(minixr.Dataset({"tas": (("lat", "lon"), np.zeros((2, 4), dtype=np.float32))},
                                              coords={"lat": np.array([0.0, 0.5]), "lon": np.arange(4) * 0.5}), q, "popwt", "hierid", {})


def test_engine_arguments_are_checked_before_any_device_work():
    """engine.quantile_select checks X first, which a host array fails."""
    from climate_toolbox_amd import engine
    with pytest.raises((TypeError, ValueError)):
        engine.quantile_select(np.zeros((3, 4), dtype=np.float32), [0, 3], [0, 1, 2], 0.0, [0.5])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_equals_numpy_quantile(dtype):
    """On float64 input the linear form agrees with np.quantile to a few ulp (NumPy's lerp is arranged differently); lower / higher
    are np.sort's elements exactly, in either dtype; q = 0 / 1 are the minimum / maximum; ties, +-0 and +-inf included."""
    rng = np.random.default_rng(17)
    T, n = 41, 9
    X = rng.uniform(250.0, 310.0, (T, n))
    X[:, 1] = rng.integers(-3, 4, T)                                              # ties
    X[::2, 2], X[1::2, 2] = 0.0, -0.0
    X[3, 3], X[7, 3] = np.inf, -np.inf
    X[5:, 4] = np.nan                                                             # m = 5
    X[:, 5] = np.nan                                                              # m = 0
    X = X.astype(dtype)
    q = [0.0, 0.05, 1.0 / 3.0, 0.5, 0.9, 0.95, 1.0, 0.5]
    rb, rows = [0, T, T], np.arange(T)
    lin, low, high = (quantile_ref(X, rb, rows, 0.0, q, m) for m in ("linear", "lower", "higher"))
    assert lin.dtype == dtype and lin.shape == (8, 2, n) and np.isnan(lin[:, 1]).all() and np.isnan(lin[:, 0, 5]).all()
    for j in (0, 1, 2, 4, 6, 7, 8):
        v = np.sort(X[~np.isnan(X[:, j]), j])
        want = np.quantile(v.astype(np.float64), q)
        np.testing.assert_allclose(lin[:, 0, j].astype(np.float64), want, rtol=4e-16 if dtype == np.float64 else 6e-8, atol=0)
        h = (len(v) - 1) * np.asarray(q)
        np.testing.assert_array_equal(low[:, 0, j], v[np.floor(h).astype(int)])
        np.testing.assert_array_equal(high[:, 0, j], v[np.ceil(h).astype(int)])
        assert lin[0, 0, j] == v[0] and lin[6, 0, j] == v[-1]
    assert low[0, 0, 3] == -np.inf and high[6, 0, 3] == np.inf and lin[3, 0, 3] == np.sort(X[:, 3])[20]
    if dtype == np.float64:                                                       # (in float32 the sum is rounded once, with the offset in it)
        np.testing.assert_array_equal(quantile_ref(X, rb, rows, -273.15, q)[:, 0, 0], lin[:, 0, 0] - 273.15)


def test_ref_by_hand():
    """one cell, rows 0..5: 1 5 2 NaN 4 3 -> v = 1 2 3 4 5.  The median is 3; q = 0.3: h = 1.2 -> 2 + (3 - 2) * 0.2 (float64
    arithmetic), lower 2, higher 3.  A row listed twice counts twice; a row outside the field and a day out of season do not count;
    a null window and an empty list give NaN; a list longer than max_rows is NaN."""
    X = np.array([[1.0, 5.0, 2.0, np.nan, 4.0, 3.0]]).T
    rb, rows = [0, 6], np.arange(6)
    g = np.float64(4) * np.float64(0.3) - 1.0
    assert quantile_ref(X, rb, rows, 0.0, [0.5, 0.3, 0, 1])[:, 0, 0].tolist() == [3.0, 2.0 + 1.0 * g, 1.0, 5.0]
    assert quantile_ref(X, rb, rows, 0.0, [0.3], "lower")[0, 0, 0] == 2.0 and quantile_ref(X, rb, rows, 0.0, [0.3], "higher")[0, 0, 0] == 3.0
    assert quantile_ref(X, rb, rows, -1.0, [0.5])[0, 0, 0] == 2.0
    assert quantile_ref(X, [0, 7], [0, 1, 2, 3, 4, 5, 1], 0.0, [0.5])[0, 0, 0] == 3.5             # 1 2 3 4 5 5
    assert quantile_ref(X, [0, 8], [0, 1, 2, 3, 4, 5, -1, 6], 0.0, [0.5])[0, 0, 0] == 3.0         # rows -1 and 6 are not in the field
    doy = np.arange(10, 16)
    assert quantile_ref(X, rb, rows, 0.0, [0.5], doy=doy, windows=np.array([12 | 15 << 10]))[0, 0, 0] == 3.0      # 2 NaN 4 3
    assert quantile_ref(X, rb, rows, 0.0, [1.0], doy=doy, windows=np.array([12 | 15 << 10]))[0, 0, 0] == 4.0
    assert np.isnan(quantile_ref(X, rb, rows, 0.0, [0.5], doy=doy, windows=np.array([WIN_NULL]))).all()
    assert np.isnan(quantile_ref(X, [0, 0], rows, 0.0, [0.5])).all()
    assert np.isnan(quantile_ref(X, rb, rows, 0.0, [0.5], max_rows=5)).all() and quantile_ref(X, rb, rows, 0.0, [0.5], max_rows=6)[0, 0, 0] == 3.0
    one = np.array([[7.0]])
    assert quantile_ref(one, [0, 1], [0], 0.0, [0, 0.37, 1])[:, 0, 0].tolist() == [7.0, 7.0, 7.0]      # m = 1: h = 0 for every level


def test_the_long_shape():
    """tests/quantile_ref.py's long shape is what tests/test_gpu_quantile.py says it gives the kernel: T = 1040; periods of 255,
    256, 257, 365, 366, 512, 513, 1023, 1024 and 0 entries; every list distinct rows of 0..1029 in no ascending order, but for the
    one that names one row twice; rows 1030.. in no list (and +inf); the six kinds of column at n = 17 and 33; the season that
    leaves a cell of a 1024-entry period fewer than 8 valid entries."""
    rb, rows = QR.long_lists()
    lens = np.diff(rb)
    assert QR.LONG_T == 1040 and list(lens) == [255, 256, 257, 365, 366, 512, 513, 1023, 1024, 0] == list(QR.LONG_LENGTHS)
    assert rb[0] == 0 and rb[-1] == len(rows) and rows.min() >= 0 and rows.max() < QR.LONG_LISTED == 1030
    assert lens.max() == QR.QUANT_ROWS_MAX and any(L % 8 != 0 and L % 16 != 0 for L in lens) and (lens > 512).sum() >= 3
    twice = []
    for p, L in enumerate(lens):
        lst = rows[rb[p]:rb[p + 1]]
        if L:
            assert (np.diff(lst) < 0).sum() > L // 4, p                           # not ascending: entry index != row index
            assert not np.array_equal(lst, np.arange(L)), p
        if len(set(lst.tolist())) != L:
            assert len(set(lst.tolist())) == L - 1
            twice.append(p)
    assert twice == [QR.LONG_TWICE]
    rb2, rows2 = QR.long_lists()
    assert np.array_equal(rb, rb2) and np.array_equal(rows, rows2)                # seeded
    for dtype in (np.float32, np.float64):
        for n in (17, 33):
            X = QR.long_field(n, dtype)
            assert X.shape == (1040, n) and X.dtype == dtype and np.isposinf(X[1030:]).all() and not np.isinf(X[:1030]).any()
            m = QR.valid_counts(X, rb, rows)
            kinds = {k: [j for j in range(n) if QR.LONG_KINDS[j % 6] == k] for k in QR.LONG_KINDS}
            assert all(kinds[k] for k in kinds)
            full = lens[:, None]
            for k in "abcf":
                assert (m[:, kinds[k]] == full).all(), k
            assert (m[:, kinds["e"]] == 0).all()
            d = m[:-1, kinds["d"]]
            assert (d > 0).all() and (d < full[:-1]).all()                        # strictly between 0 and L, every non-empty period
            assert (m[:-1, kinds["d"]] != m[:-1, [j - 1 for j in kinds["d"]]]).all()      # and not the neighbouring cell's m
            a, b, c, f = (X[:1030, kinds[k][0]] for k in "abcf")
            assert (a < 0).any() and (a > 0).any() and len(set(a.tolist())) > 1000
            assert set(b.tolist()) == {-0.5, -0.25, 0.0, 0.25, 0.5} and len(set(c.tolist())) == 1
            tiny = np.finfo(dtype).tiny
            assert np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all() and ((f != 0) & (np.abs(f) < tiny)).any()
            for p in (7, 8):                                                      # 1023 and 1024 entries: ties at the median
                col = np.sort(X[rows[rb[p]:rb[p + 1]], kinds["b"][0]])
                assert (col == col[(len(col) - 1) // 2]).sum() >= 100, p
            doy, win = QR.long_season(n)
            assert doy.min() == 1 and doy.max() == 366 and np.array_equal(doy, 1 + np.arange(1040) % 366) and win.shape == (n,)
            assert (win == (0 | 1023 << 10)).any() and (win & WIN_NULL).any() and (win & WIN_INVERT).any()
            ms = QR.valid_counts(X, rb, rows, doy, win)
            assert ((ms[8] > 0) & (ms[8] < 8)).any() and (ms[8] == 1024).any() and (ms[8] == 0).any()
            assert (ms <= m).all() and len(set(ms[8].tolist())) >= 6
    # the restatement on it: the median of the all-equal column, and of the tied one, by hand
    X = QR.long_field(17, np.float64)
    want = quantile_ref(X, rb, rows, 0.0, [0.5], "linear")
    assert want.shape == (1, 10, 17) and np.isnan(want[0, 9]).all() and np.isnan(want[0, :, 4]).all()
    assert (want[0, :9, 2] == 287.65).all() and set(want[0, :9, 1].tolist()) <= {-0.5, -0.25, 0.0, 0.25, 0.5}
