"""Period quantiles on the GPU (run with -m gpu): wagg_quantile_select_* through engine.quantile_select against the NumPy
restatement tests/quantile_ref.py, and tas_quantile_aggregate on a segment table against that restatement aggregated by the fp64
oracle.

At the kernel layer results are compared EXACTLY -- equal as numbers, NaN exactly where the restatement has NaN: the selection is
exact and the interpolation is three separately rounded fp64 operations on both sides.  Only the weighted mean of the public call
rounds.  The kernel cases use the rolling extremes' small shape -- T = 23 rows, three periods of 9, 8 and 0 entries, a gap at row
4 -- and the row-list layout tests' one list of 70 entries (rows 0..69 without row 41, row 5 listed twice): more than one load per
lane in phase 1 (8 | 16 entries a pass) and more than 64 entries.

The kernel's real workload -- a year of 365 or 366 entries, up to its limit of 1024, 128 KiB of LDS -- is the LONG SHAPE of
tests/quantile_ref.py (T = 1040; ten periods of 255 .. 1024 and 0 entries in one call; tests/test_quantile_host.py checks the shape
itself) at n = 17 and 33, RL.LONG (512 entries over 64 rows, every row eight times) and a public call over 2004 and 2005.  Their
references are computed once per (element type, n, method, offset, season) and shared (``_long_want``)."""
import functools

import numpy as np
import pytest

from tests import rowlist_layout as RL
from tests import quantile_ref as QR
from tests.quantile_ref import quantile_ref
from tests.rolling_ref import WIN_INVERT, WIN_NULL, in_season
from tests.test_gpu_packed_totals import _Sparse, segment_plans  # noqa: F401
from tests.test_gpu_rolling import RB, ROWS, T, _Worst, _exact, _strided
from tests.test_gpu_seasons import _mask_TG, _seasons_for

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 31, 32, 33, 65, 1029)       # one short of, on and one past the fp64 (16) and fp32 (32) tile; several tiles
Q8 = [0.0, 0.05, 1.0 / 3.0, 0.5, 0.9, 0.95, 1.0, 0.5]
Q16 = [0.5, 0.0, 1.0, 0.05, 0.95, 0.99, 0.01, 1.0 / 3.0, 2.0 / 3.0, 0.25, 0.75, 0.5, 0.1, 0.9, 0.125, 0.999]
METHODS = ("linear", "lower", "higher")
OPEN = 0 | 1023 << 10
SHAPES = ((T, RB, ROWS), RL.SPLIT)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _field(Tn, n, dtype, seed):
    """values of both signs with fractions, a tie per cell (rows 1 and 2 hold the same value)"""
    X = np.random.default_rng(seed).uniform(-30.0, 45.0, (Tn, n))
    X[2] = X[1]
    return X.astype(dtype)


def _same(torch, a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


def _dev_lists(torch, rb, rows):
    return torch.tensor(np.asarray(rb), dtype=torch.int32, device="cuda"), torch.tensor(np.asarray(rows), dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_quantiles_equal_the_restatement(torch_cuda, dtype, n):
    """Eight levels (0, 1, a duplicate, 1/3) with all three methods, offset 0 and -273.15, on contiguous rows and on pitched ones
    (ldx = n + 1), with max_rows equal to the longest list and equal to 1024: every plane equals the restatement exactly; the empty
    period is NaN in every plane; the status word stays 0."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    for (Tn, rb, rows) in SHAPES:
        X = _field(Tn, n, dtype, seed=Tn + n)
        P, longest = len(rb) - 1, int(np.diff(rb).max())
        for method in METHODS:
            for off in (0.0, -273.15):
                want = quantile_ref(X, rb, rows, off, Q8, method)
                for pad in (0, 1):
                    Xd = _strided(torch, X, pad)
                    for max_rows in (longest, 1024):
                        what = (Tn, n, pad, method, off, max_rows)
                        got, st = engine.quantile_select(Xd, rb, rows, off, Q8, method=method, max_rows=max_rows)
                        assert got.shape == (8, P, n) and got.dtype == tdt and int(st.item()) == 0, what
                        _exact(got, want, what)
                        if Tn == T:
                            assert torch.isnan(got[:, 2]).all() and not torch.isnan(got[:, :2]).any(), what
        auto, _ = engine.quantile_select(Xd, rb, rows, -273.15, Q8, method="higher")       # max_rows=None: the longest list
        _exact(auto, want, (Tn, n, "max_rows=None"))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_key_map_orders_every_kind_of_value(torch_cuda, dtype):
    """Cells built to break an order-preserving key or a short bisection: 0 both signs; 1 only -0.0 and +0.0; 2 denormals of both
    signs around zero; 3 two values one ulp apart; 4 values that differ in their LOW bits only (fp64: the low 32 bits -- a bisection
    that stops after 32 sweeps cannot tell them apart); 5 small integers with many ties (the c_le rule); 6 all equal; 7 huge and
    tiny magnitudes.  Period 0 holds all 12 rows, period 1 one row (m = 1), period 2 two rows (m = 2)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    Tn, n = 12, 8
    eps = np.finfo(dtype).eps
    tiny = np.finfo(dtype).smallest_subnormal
    X = np.zeros((Tn, n), dtype=dtype)
    X[:, 0] = [3.5, -2.25, 0.75, -0.5, 10.0, -10.0, 1e-3, -1e-3, 2.0, -2.0, 0.0, 7.0]
    X[:, 1] = [0.0, -0.0] * 6
    X[:, 2] = [tiny, -tiny, 3 * tiny, 0.0, -0.0, -5 * tiny, 2 * tiny, np.finfo(dtype).tiny, -np.finfo(dtype).tiny, tiny, 0.0, -2 * tiny]
    X[:, 3] = [1.0, 1.0 + eps] * 6
    X[:, 4] = dtype(1.0) + dtype(eps) * np.array([5, 3, 9, 1, 7, 0, 11, 2, 8, 4, 10, 6], dtype=dtype)
    X[:, 5] = [2, 1, 2, 3, 2, 1, 3, 2, 2, 1, 2, 3]
    X[:, 6] = 287.65
    X[:, 7] = [np.finfo(dtype).max, -np.finfo(dtype).max, 1.0, -1.0, tiny, -tiny, 1e30, -1e30, 1e-30, -1e-30, 0.5, -0.5]
    if dtype == np.float64:
        low = np.ascontiguousarray(X[:, 4]).view(np.uint64)
        assert len(set((low >> np.uint64(32)).tolist())) == 1 and len(set(low.tolist())) == Tn      # only the low 32 bits differ
    rb, rows = np.array([0, 12, 13, 15]), np.concatenate([np.arange(12)[::-1], [4], [9, 2]])
    q = Q8 + [0.25, 0.75, 0.6, 0.0625]
    for method in METHODS:
        want = quantile_ref(X, rb, rows, 0.0, q, method)
        assert not np.isnan(want).any()
        for pad in (0, 1):
            got, st = engine.quantile_select(_strided(torch, X, pad), rb, rows, 0.0, q, method=method)
            assert int(st.item()) == 0
            _exact(got, want, (method, pad))
    mid = quantile_ref(X, rb, rows, 0.0, [0.5], "lower")[0, 0]
    assert mid[3] == 1.0 and mid[4] == dtype(1.0) + dtype(5 * eps) and mid[5] == 2.0 and mid[6] == dtype(287.65)
    assert quantile_ref(X, rb, rows, 0.0, [0.5], "linear")[0, 2, 0] == dtype((float(X[9, 0]) + float(X[2, 0])) / 2)      # m = 2


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_validity_nan_seasons_repeats_and_rows_outside(torch_cuda, dtype):
    """On a 16 x 32 grid (512 cells, 16 | 32 tiles) with growing seasons of every kind per cell and NaN days, the number of valid
    entries differs between neighbouring cells of one tile and is 0 for some; a row is listed twice; under checked=True two row
    indices outside [0, T) are skipped; the pad column of the pitched field is NaN and never reaches a result.  Against the
    restatement on the field masked in NumPy by tests/test_gpu_seasons.py's mask -- and against the restatement's own season rule."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, periods
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=41)
    Tn, G = c.T, c.G
    rng = np.random.default_rng(8)
    X = c.tas.reshape(Tn, G).copy()
    X[rng.uniform(size=X.shape) < 0.1] = np.nan
    gd, z1, z2 = _seasons_for(c, seed=Tn)
    win = np.ascontiguousarray(pkg.season_windows(gd)[0][:c.nlat].reshape(-1))
    doy = pkg.day_of_year(c.time)
    mask = _mask_TG(z1, z2, doy)
    _, rb, rows = periods.period_rows(c.time, "month")
    rows = np.concatenate([rows[:31], [7], rows[31:]])                            # row 7 twice in January
    rb = np.array([0, 32, len(rows)])
    masked = np.where(mask == 1, X, np.nan).astype(dtype)
    m = (~np.isnan(masked[rows[:32]])).sum(axis=0)
    assert (m == 0).any() and (np.diff(m[:16]) != 0).any() and m.max() > 20
    buf = torch.full((Tn, G + 1), float("nan"), dtype=torch.from_numpy(X[:1]).dtype, device="cuda")      # the pad column is NaN
    buf[:, :G] = torch.from_numpy(X).cuda()
    for Xd in (torch.from_numpy(X).cuda(), buf[:, :G]):
        for method in ("linear", "higher"):
            got, st = engine.quantile_select(Xd, rb, rows, -273.15, Q8, method=method, doy=doy, windows=win)
            assert int(st.item()) == 0
            _exact(got, quantile_ref(masked, rb, rows, -273.15, Q8, method), (method, "masked"))
    _exact(got, quantile_ref(X, rb, rows, -273.15, Q8, "higher", doy, win), "season rule")
    assert torch.isnan(got[:, 0, torch.from_numpy(m == 0).cuda()]).all()
    # row indices outside the field, on device lists the library does not look at
    wild = np.concatenate([rows[:10], [-1, Tn, 2 ** 31 - 1], rows[10:]])
    rbw = np.array([0, 35, len(wild)])
    drb, drw = _dev_lists(torch, rbw, wild)
    got, st = engine.quantile_select(buf[:, :G], drb, drw, 0.0, Q8, max_rows=64, doy=doy, windows=win, checked=True)
    assert int(st.item()) == 0
    _exact(got, quantile_ref(masked, rb, rows, 0.0, Q8), "rows outside")
    with pytest.raises(engine.WaggError, match="row index"):
        engine.quantile_select(buf[:, :G], drb, drw, 0.0, Q8, max_rows=64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_infinity_sets_the_status_word(torch_cuda, dtype):
    """A listed, in-season +inf (or -inf) is a valid value -- the maximum (minimum) -- and sets bit 0; out of season, or in a row no
    list names (row 4, row 20), it sets nothing and changes nothing."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 5
    X = _field(T, n, dtype, seed=3)
    doy = np.arange(100, 100 + T)
    win = np.full(n, 100 | 110 << 10, dtype=np.int32)                             # rows 0..10 in season
    for v in (np.inf, -np.inf):
        for t, listed, in_win in ((6, True, True), (14, True, False), (4, False, True), (20, False, False)):
            Xi = X.copy()
            Xi[t, 3] = v
            for kw in (dict(doy=doy, windows=win), {}):
                counted = listed and (in_win or not kw)
                got, st = engine.quantile_select(torch.from_numpy(Xi).cuda(), RB, ROWS, 0.0, [0.0, 0.5, 1.0], **kw)
                assert int(st.item()) == (1 if counted else 0), (v, t, bool(kw))
                _exact(got, quantile_ref(Xi, RB, ROWS, 0.0, [0.0, 0.5, 1.0], "linear", kw.get("doy"), kw.get("windows")), (v, t))
                if counted:
                    assert float(got[2 if v > 0 else 0, 0 if t < 10 else 1, 3]) == v


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [33, 1029])
def test_a_list_longer_than_max_rows_is_confined(torch_cuda, dtype, n):
    """checked=True with max_rows one short of the longest list (9): that period is NaN in every plane and bit 1 of the status word
    is set; the period of 8 entries and the empty one are exact; the sentinel behind ``out`` is untouched.  Without checked=True
    the library's look at the device lists rejects the call; max_rows outside 1..1024 is the binding's ValueError."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    X = _field(T, n, dtype, seed=n)
    Xd = torch.from_numpy(X).cuda()
    drb, drw = _dev_lists(torch, RB, ROWS)
    size = 8 * 3 * n
    big = torch.full((size + RL.GUARD,), 12345.0, dtype=Xd.dtype, device="cuda")
    out = big[:size].view(8, 3, n)
    got, st = engine.quantile_select(Xd, drb, drw, 0.0, Q8, max_rows=8, checked=True, out=out)
    assert got.data_ptr() == big.data_ptr() and int(st.item()) == 2
    assert bool((big[size:] == 12345.0).all())
    want = quantile_ref(X, RB, ROWS, 0.0, Q8, max_rows=8)
    assert np.isnan(want[:, 0]).all() and not np.isnan(want[:, 1]).any()
    _exact(got, want, "confined")
    full, st = engine.quantile_select(Xd, drb, drw, 0.0, Q8, max_rows=9, checked=True)
    assert int(st.item()) == 0
    _exact(full, quantile_ref(X, RB, ROWS, 0.0, Q8), "fits")
    with pytest.raises(engine.WaggError, match="max_rows"):
        engine.quantile_select(Xd, drb, drw, 0.0, Q8, max_rows=8)
    _exact(engine.quantile_select(Xd, drb, drw, 0.0, Q8)[0], quantile_ref(X, RB, ROWS, 0.0, Q8), "device lists, max_rows=None")
    for bad in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="max_rows"):
            engine.quantile_select(Xd, RB, ROWS, 0.0, Q8, max_rows=bad)
    with pytest.raises(ValueError, match="quantile"):
        engine.quantile_select(Xd, RB, ROWS, 0.0, [0.5] * 17)
    with pytest.raises(ValueError, match="quantile"):
        engine.quantile_select(Xd, RB, ROWS, 0.0, [1.5])
    with pytest.raises(ValueError, match="method"):
        engine.quantile_select(Xd, RB, ROWS, 0.0, [0.5], method="nearest")
    with pytest.raises(ValueError, match="go together"):
        engine.quantile_select(Xd, RB, ROWS, 0.0, [0.5], doy=np.arange(T))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planes_and_extremes_bit_for_bit(torch_cuda, dtype):
    """Plane k of a 16-level call -- unsorted, with duplicates: two quantiles a lane in fp32 -- is the one-level call bit for bit;
    two runs are bit-equal; q = 1 / q = 0 are engine.rolling_reduce's W = 1 maximum / minimum on the same lists.  Under a season
    and without, contiguous and pitched, both shapes."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    n = 257
    assert len(Q16) == _lib.QUANT_MAX
    for (Tn, rb, rows) in SHAPES:
        X = _field(Tn, n, dtype, seed=7)
        X[3, ::5] = np.nan
        doy = np.arange(100, 100 + Tn)
        win = np.where(np.arange(n) % 3 == 0, OPEN, 101 | 130 << 10).astype(np.int32)
        for pad in (0, 1):
            Xd = _strided(torch, X, pad)
            for kw in (dict(doy=doy, windows=win), {}):
                for method in METHODS:
                    got, st = engine.quantile_select(Xd, rb, rows, -273.15, Q16, method=method, **kw)
                    assert int(st.item()) == 0
                    for k, qk in enumerate(Q16):
                        one, _ = engine.quantile_select(Xd, rb, rows, -273.15, [qk], method=method, **kw)
                        assert _same(torch, got[k], one[0]), (Tn, pad, method, k)
                    assert _same(torch, got[0], got[11]) and _same(torch, engine.quantile_select(Xd, rb, rows, -273.15, Q16, method=method, **kw)[0], got)
                    hi, _ = engine.rolling_reduce(Xd, rb, rows, -273.15, [1], stat="max", of="mean", **kw)
                    lo, _ = engine.rolling_reduce(Xd, rb, rows, -273.15, [1], stat="min", of="mean", **kw)
                    assert _same(torch, got[2], hi[0]) and _same(torch, got[1], lo[0]), (Tn, pad, method)
                _exact(got, quantile_ref(X, rb, rows, -273.15, Q16, "higher", kw.get("doy"), kw.get("windows")), (Tn, pad))


@pytest.mark.parametrize("dtype,kelvin", [(np.float32, True), (np.float64, False)])
def test_public_call(torch_cuda, segment_plans, dtype, kelvin):
    """tas_quantile_aggregate on a small synthetic grid with a segment table -- a Kelvin-shifted fp32 field, a plain fp64 one --
    for period="year" (40 days) and "month" (31 + 9), cells="all" and "referenced", with and without a season: against the
    restatement of the per-cell quantiles aggregated by the fp64 oracle of (X W) / (1' W), within 1e-4 (fp32) / 1e-6 (fp64) of the
    same aggregation of the absolute parts (the largest ratio to that bound is printed).  One referenced cell is NaN throughout:
    its NaN meets the contraction (it counts 0, its weight stays in the denominator -- the oracle's rule too).  Dims, the quantile
    coordinate, the attributes, results_on_device(), more than 16 levels in two launches; a counted +inf, a power variable,
    period=None, a bad q and a period of more than 1024 days raise."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, minixr, periods
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_poly, tas_quantile_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=29)
    Tn = c.T
    q = [0.5, 0.05, 0.95, 0.5, 1.0]
    field = c.tas.copy()
    flat = field.reshape(Tn, c.G)
    flat[::3, int(c.cell[1])] = np.nan
    flat[:, int(c.cell[2])] = np.nan
    off = -273.15 if kelvin else 0.0
    gd, z1, z2 = _seasons_for(c, seed=Tn)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time))

    def ds(device=True, f=None):
        d = c.dataset(torch, device=device, tas=field if f is None else f)
        return convert_kelvin_to_celsius(d, "tas") if kelvin else d

    worst = _Worst()
    for period in ("year", "month"):
        _, rb, rows = periods.period_rows(c.time, period)
        P = len(rb) - 1
        assert P == (1 if period == "year" else 2)
        for season in (None, sw):
            src = flat if season is None else np.where(mask == 1, flat, np.nan).astype(dtype)      # out of season = not valid
            for method in (("linear", "lower") if period == "year" else ("linear", "higher")):
                what = (period, season is not None, method)
                cells = quantile_ref(src, rb, rows, off, q, method).astype(np.float64)            # (n_q, P, G)
                assert np.isnan(cells[:, :, int(c.cell[2])]).all()
                want = np.stack([O.agg_coded(cells[k], c.cell, c.code, c.w_eff, c.R) for k in range(len(q))])
                scale = np.stack([O.agg_coded(np.abs(np.nan_to_num(cells[k], nan=0.0)), c.cell, c.code, c.w_eff, c.R) for k in range(len(q))])
                call = lambda d=None, **kw: tas_quantile_aggregate(d if d is not None else ds(), q, "popwt", "reg", c.df, method=method,
                                                                   period=period, season=season, **kw)
                out = call()
                v = out["tas-quantile"]
                assert v.dims == ("quantile", "period", "reg") and v.attrs["method"] == method, what
                assert v.attrs.get("units") == ("C" if kelvin else None)
                assert out["quantile"].values.dtype == np.float64 and list(out["quantile"].values) == q
                assert len(out["period"].values) == P
                got = v.values
                assert isinstance(v.data, np.ndarray) and got.dtype == dtype and got.shape == (len(q), P, c.R)
                assert np.isnan(got[:, :, c.R - 1]).all()                                 # the region without weight
                worst.ok(got, want, scale, c.rtol, what)
                np.testing.assert_array_equal(got[0], got[3])                             # the duplicate level
                ref = call(cells="referenced")["tas-quantile"].values
                worst.ok(ref, want, scale, c.rtol, what + ("referenced",))
                worst.ok(ref, got.astype(np.float64), scale, c.rtol, what + ("referenced vs all",))
                np.testing.assert_array_equal(call(ds(device=False))["tas-quantile"].values, got)
    print("quantile public call %s: largest |got - ref| / (RTOL * A) = %.3g" % (np.dtype(dtype).name, worst.ratio))
    with pkg.results_on_device():
        on = call()
        assert isinstance(on["tas-quantile"].data, torch.Tensor) and on["tas-quantile"].data.is_cuda
        assert isinstance(call(ds(device=False))["tas-quantile"].data, np.ndarray)
    np.testing.assert_array_equal(on["tas-quantile"].values, got)
    np.testing.assert_array_equal(call(varname="typical")["typical"].values, got)
    # more than 16 levels: 16, then 2, joined in the caller's order
    ran = []
    real = engine.quantile_select
    many_q = [k / 17.0 for k in range(18)]
    many = lambda w: tas_quantile_aggregate(ds(), w, "popwt", "reg", c.df, period="month")["tas-quantile"].values
    try:
        engine.quantile_select = lambda *a, **k: (ran.append(len(a[4])), real(*a, **k))[1]
        v18 = many(many_q)
    finally:
        engine.quantile_select = real
    assert ran == [16, 2] and v18.shape == (18, 2, c.R)
    np.testing.assert_array_equal(v18[:16], many(many_q[:16]))
    np.testing.assert_array_equal(v18[16:], many(many_q[16:]))
    # what raises
    hit = field.copy()
    hit.reshape(Tn, c.G)[3, int(c.cell[0])] = np.inf
    for cells_kw in ("all", "referenced"):
        with pytest.raises(ValueError, match="inf"):
            tas_quantile_aggregate(ds(f=hit), [0.5, 1.0], "popwt", "reg", c.df, period="year", cells=cells_kw)
    with pytest.raises(ValueError, match="plain"):
        tas_quantile_aggregate(tas_poly(c.dataset(torch, device=False, tas=field), 2, "tas-poly-2"), q, "popwt", "reg", c.df, tas="tas-poly-2")
    with pytest.raises(ValueError, match="needs period="):
        tas_quantile_aggregate(ds(), q, "popwt", "reg", c.df, period=None)
    for bad in ([0.5, 1.5], [float("nan")], [True], []):
        with pytest.raises(ValueError, match="q must be"):
            tas_quantile_aggregate(ds(), bad, "popwt", "reg", c.df)
    long_T = 1025
    long_ds = minixr.Dataset({"tas": (("time", "lat", "lon"), np.zeros((long_T, c.nlat, c.nlon), dtype=dtype))},
                             coords={"time": np.datetime64("2001-01-01") + np.arange(long_T), "lat": c.lat, "lon": c.lon})
    with pytest.raises(ValueError, match="1025 days.*at most 1024"):
        tas_quantile_aggregate(long_ds, q, "popwt", "reg", c.df, period=np.zeros(long_T, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# lists as long as the workload's: a year, the limit of 1024 entries, every entry of LDS beyond 64 KiB
# ---------------------------------------------------------------------------------------------------------------------------------
LONG_NS = (17, 33)                                # fp64: 2 and 3 tiles; fp32: 1 and 2, the last holding one cell
LONG_RB, LONG_ROWS = QR.long_lists()
EMPTY = len(QR.LONG_LENGTHS) - 1


@functools.lru_cache(maxsize=None)
def _long_field(n, dtype):
    X = QR.long_field(n, dtype)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _long_want(n, dtype, method, off, season):
    """the restatement on the long shape, once per case (read-only: shared by the tests below)"""
    sk = QR.long_season(n) if season else (None, None)
    want = quantile_ref(_long_field(n, dtype), LONG_RB, LONG_ROWS, off, Q16, method, *sk)
    want.setflags(write=False)
    return want


def _inf_padded(torch, host, pad):
    """a device tensor with row stride n + pad whose pad columns hold +inf: a lane of the last, partial tile that read past n
    would raise bit 0 of the status word"""
    Tn, n = host.shape
    dev = torch.from_numpy(np.array(host)).cuda()                                 # (a copy: the cached fields are read-only)
    buf = torch.full((Tn, n + pad), float("inf"), dtype=dev.dtype, device="cuda")
    buf[:, :n] = dev
    out = buf[:, :n]
    assert out.stride(0) == n + pad
    return out


def _season_kw(n, season):
    if not season:
        return {}
    doy, win = QR.long_season(n)
    return dict(doy=doy, windows=win)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", LONG_NS)
def test_long_lists_equal_the_restatement(torch_cuda, dtype, n):
    """The long shape in ONE call, 16 levels, all three methods, offset 0 and -273.15, with a season (doy = 1 + t % 366, every
    kind of window on every kind of column; some cell keeps fewer than 8 of a 1024-entry list) and without, on contiguous rows and
    on ldx = n + 1 with +inf in the pad column, max_rows = 1024 -- which IS the longest list of this call -- and max_rows=None:
    every plane equals the restatement exactly, the empty period and the all-NaN columns are NaN in every plane, and the status
    word stays 0 although rows 1030.. and the pad hold +inf."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    X = _long_field(n, dtype)
    P = len(LONG_RB) - 1
    assert int(np.diff(LONG_RB).max()) == 1024
    nan_cols = [j for j in range(n) if QR.LONG_KINDS[j % 6] == "e"]
    for season in (False, True):
        kw = _season_kw(n, season)
        for pad in (0, 1):
            Xd = _inf_padded(torch, X, pad)
            for method in METHODS:
                for off in (0.0, -273.15):
                    what = (n, season, pad, method, off)
                    got, st = engine.quantile_select(Xd, LONG_RB, LONG_ROWS, off, Q16, method=method, max_rows=1024, **kw)
                    assert got.shape == (16, P, n) and int(st.item()) == 0, what
                    _exact(got, _long_want(n, dtype, method, off, season), what)
                    assert torch.isnan(got[:, EMPTY]).all() and torch.isnan(got[:, :, nan_cols]).all(), what
            auto, st = engine.quantile_select(Xd, LONG_RB, LONG_ROWS, -273.15, Q16, method="higher", **kw)      # max_rows=None
            assert int(st.item()) == 0
            _exact(auto, _long_want(n, dtype, "higher", -273.15, season), (n, season, pad, "max_rows=None"))
            assert not torch.isnan(auto[:, :EMPTY, 0]).any()                      # (column 0: continuous, open all year)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_row_eight_times(torch_cuda, dtype):
    """RL.LONG -- ONE list of 512 entries over 64 rows, every row eight times: every value is an eightfold tie, so v[lo + 1] is
    v[lo] for seven ranks of eight (the c_le rule) -- at n = 33: the result equals the restatement exactly, and for every level
    the "lower" and the "higher" plane bracket the "linear" one."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    Tn, rb, rows = RL.LONG
    n = 33
    X = _field(Tn, n, dtype, seed=64)
    X[5, ::4] = np.nan                                                            # m = 504 in every fourth cell
    planes = {}
    for method in METHODS:
        for pad in (0, 1):
            got, st = engine.quantile_select(_inf_padded(torch, X, pad), rb, rows, -273.15, Q16, method=method, max_rows=512)
            assert int(st.item()) == 0
            _exact(got, quantile_ref(X, rb, rows, -273.15, Q16, method), (method, pad))
        planes[method] = got.cpu().numpy()
    assert not np.isnan(planes["linear"]).any()
    assert (planes["lower"] <= planes["linear"]).all() and (planes["linear"] <= planes["higher"]).all()
    assert (planes["lower"] < planes["higher"]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_confinement_at_the_limit(torch_cuda, dtype):
    """Device lists of 1024 and 1025 entries (the second: the first plus one repeated row, T unchanged) with checked=True and
    max_rows=1024: the 1025-entry period is NaN in every plane and the status word is 2, the 1024-entry period -- all 128 KiB of
    LDS -- is exact, a sentinel behind ``out`` is untouched.  Without checked=True the library's look at the lists rejects the
    call; max_rows=None with a host list of 1025 entries is the binding's ValueError."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 33
    X = _long_field(n, dtype)
    full = LONG_ROWS[LONG_RB[8]:LONG_RB[9]]
    assert len(full) == 1024 and len(set(full.tolist())) == 1024
    rb, rows = np.array([0, 1024, 2049]), np.concatenate([full, full, [full[3]]])
    Xd = torch.from_numpy(np.array(X)).cuda()
    drb, drw = _dev_lists(torch, rb, rows)
    size = 16 * 2 * n
    big = torch.full((size + RL.GUARD,), 12345.0, dtype=Xd.dtype, device="cuda")
    out = big[:size].view(16, 2, n)
    got, st = engine.quantile_select(Xd, drb, drw, 0.0, Q16, max_rows=1024, checked=True, out=out)
    assert got.data_ptr() == big.data_ptr() and int(st.item()) == 2
    assert bool((big[size:] == 12345.0).all())
    want = quantile_ref(X, rb, rows, 0.0, Q16, max_rows=1024)
    assert np.isnan(want[:, 1]).all() and not np.isnan(want[:, 0, :3]).any() and torch.isnan(got[:, 1]).all()
    _exact(got, want, "confined at 1025")
    np.testing.assert_array_equal(want[:, 0], _long_want(n, dtype, "linear", 0.0, False)[:, 8])
    with pytest.raises(engine.WaggError, match="max_rows"):
        engine.quantile_select(Xd, drb, drw, 0.0, Q16, max_rows=1024)
    with pytest.raises(ValueError, match="1025 rows"):
        engine.quantile_select(Xd, rb, rows, 0.0, Q16)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planes_and_extremes_bit_for_bit_at_length(torch_cuda, dtype):
    """On the long shape at n = 33, under a season and without: plane k of the 16-level call is the one-level call bit for bit;
    q = 1 / q = 0 are engine.rolling_reduce's W = 1 maximum / minimum on the same lists."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 33
    Xd = _inf_padded(torch, _long_field(n, dtype), 1)
    for season in (False, True):
        kw = _season_kw(n, season)
        for method in METHODS:
            got, st = engine.quantile_select(Xd, LONG_RB, LONG_ROWS, -273.15, Q16, method=method, max_rows=1024, **kw)
            assert int(st.item()) == 0
            for k, qk in enumerate(Q16):
                one, _ = engine.quantile_select(Xd, LONG_RB, LONG_ROWS, -273.15, [qk], method=method, max_rows=1024, **kw)
                assert _same(torch, got[k], one[0]), (season, method, k)
            hi, _ = engine.rolling_reduce(Xd, LONG_RB, LONG_ROWS, -273.15, [1], stat="max", of="mean", **kw)
            lo, _ = engine.rolling_reduce(Xd, LONG_RB, LONG_ROWS, -273.15, [1], stat="min", of="mean", **kw)
            assert _same(torch, got[2], hi[0]) and _same(torch, got[1], lo[0]), (season, method)
        _exact(got, _long_want(n, dtype, "higher", -273.15, season), season)


@pytest.mark.parametrize("dtype,kelvin", [(np.float32, True), (np.float64, False)])
def test_public_call_over_real_years(torch_cuda, segment_plans, dtype, kelvin):
    """tas_quantile_aggregate(period="year") on the 16 x 32 grid and table of test_public_call with 731 daily steps from
    2004-01-01 -- a year of 366 and one of 365 entries -- for cells="all" and "referenced", with and without a season: against the
    restatement per cell aggregated by the fp64 oracle, by test_public_call's rule and rtol (the largest ratio is printed)."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import periods
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_quantile_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=31)
    Tn = c.T = 731
    c.time = np.datetime64("2004-01-01") + np.arange(Tn)
    rng = np.random.default_rng(2004)
    flat = (280 + 15 * rng.standard_normal((Tn, c.G))).astype(dtype)
    flat[::3, int(c.cell[1])] = np.nan
    flat[:, int(c.cell[2])] = np.nan
    field = flat.reshape(Tn, c.nlat, c.nlon)
    q = [0.5, 0.05, 0.95, 0.99, 1.0]
    off = -273.15 if kelvin else 0.0
    gd, z1, z2 = _seasons_for(c, seed=Tn)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time))
    _, rb, rows = periods.period_rows(c.time, "year")
    assert list(np.diff(rb)) == [366, 365]

    def ds():
        d = c.dataset(torch, tas=field)
        return convert_kelvin_to_celsius(d, "tas") if kelvin else d

    worst = _Worst()
    for season in (None, sw):
        src = flat if season is None else np.where(mask == 1, flat, np.nan).astype(dtype)
        for method in ("linear", "higher"):
            what = (season is not None, method)
            cells = quantile_ref(src, rb, rows, off, q, method).astype(np.float64)                # (n_q, 2, G)
            assert np.isnan(cells[:, :, int(c.cell[2])]).all()
            want = np.stack([O.agg_coded(cells[k], c.cell, c.code, c.w_eff, c.R) for k in range(len(q))])
            scale = np.stack([O.agg_coded(np.abs(np.nan_to_num(cells[k], nan=0.0)), c.cell, c.code, c.w_eff, c.R) for k in range(len(q))])
            for cells_kw in ("all", "referenced"):
                got = tas_quantile_aggregate(ds(), q, "popwt", "reg", c.df, method=method, period="year", season=season,
                                             cells=cells_kw)["tas-quantile"].values
                assert got.dtype == dtype and got.shape == (len(q), 2, c.R), what
                worst.ok(got, want, scale, c.rtol, what + (cells_kw,))
    print("quantile public call over 2004-2005 %s: largest |got - ref| / (RTOL * A) = %.3g" % (np.dtype(dtype).name, worst.ratio))
