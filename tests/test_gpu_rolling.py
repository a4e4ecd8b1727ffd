"""Rolling-window extremes on the GPU (run with -m gpu): wagg_rolling_reduce_* through engine.rolling_reduce against the NumPy
restatement tests/rolling_ref.py, and tas_rolling_aggregate on a segment table against that restatement aggregated by the fp64
oracle.

At the kernel layer results are compared EXACTLY -- equal as numbers, NaN exactly where the restatement has NaN: the window sums
are fp64 chains without a product, formed in the same order on both sides.  Only the weighted mean of the public call rounds.
The kernel cases use the spells' small shape -- T = 23 rows, three periods of 9, 8 and 0 entries: rows 0..9 without row 4 (a gap
inside the first period), rows 10..17 (one full ring of 8; rows 9 | 10 are consecutive across the period boundary), nothing --
and a second one that wraps the ring of 16 twice: T = 40, one period of 33 consecutive rows and one of 4."""
import numpy as np
import pytest

from tests.rolling_ref import WIN_INVERT, WIN_NULL, in_season, rolling_ref
from tests.test_gpu_packed_totals import _Sparse, segment_plans  # noqa: F401
from tests.test_gpu_seasons import _mask_TG, _seasons_for

pytestmark = pytest.mark.gpu

T = 23
RB = np.array([0, 9, 17, 17])
ROWS = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17])
T2 = 40
RB2 = np.array([0, 33, 37])
ROWS2 = np.concatenate([np.arange(2, 35), np.arange(36, 40)])
NS = (1, 3, 4, 5, 257, 1029)
OPEN = 0 | 1023 << 10
LENGTHS = [1, 2, 3, 4, 5, 8, 9, 16]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _pads(n, dtype):
    """(a pad that keeps rows 16-byte aligned: the VEC = 4 / 2 route, one that breaks the alignment: the VEC = 1 route)"""
    v = 16 // np.dtype(dtype).itemsize
    return (-n) % v, (-n) % v + 1


def _strided(torch, host, pad):
    """a device tensor with row stride n + pad"""
    Tn, n = host.shape
    buf = torch.zeros((Tn, n + pad), dtype=torch.from_numpy(host[:1]).dtype, device="cuda")
    buf[:, :n] = torch.from_numpy(host).cuda()
    out = buf[:, :n]
    assert out.stride(0) == n + pad
    return out


def _field(Tn, n, dtype, seed):
    """Kelvin-like values 250..310 with fractions (fp64 sums that depend on their order).  Designed cells, where n allows: cell 0
    is greatest on the FIRST entry of each list (rows 0 and 10), cell 1 on the LAST (rows 9 and 17), cell 2 on the entry right
    behind the gap (row 5; row 3, ahead of the gap, is second: a pair across the gap would win), cell 3 on rows 9 and 10 only --
    the two sides of the period boundary."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(250.0, 310.0, (Tn, n))
    if n > 0:
        X[[0, 10], 0] = 1000.0
    if n > 1:
        X[[9, 17], 1] = 1000.0
    if n > 2:
        X[5, 2], X[3, 2] = 1000.0, 900.0
    if n > 3:
        X[[9, 10], 3] = 1000.0
    return X.astype(dtype)


def _exact(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, "%r: %d values differ, first at (window, period, cell) %r: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_windows_equal_the_restatement(torch_cuda, dtype, n):
    """Windows 1, 2, 3, 4, 5, 8, 9, 16 in one launch (the ring of 16), max and min, mean and sum, offset 0 and -273.15, on aligned
    rows (a partial last piece for n = 1, 3, 5, 257, 1029; more than one column block for 1029) and on rows that are not 16-byte
    aligned; no season.  Window 9 exceeds every gap-free stretch of the small shape (4 + 5 | 8 entries): its plane and that of 16
    are NaN there; the empty period is NaN in every plane.  In the 33-row shape windows 9 and 16 exist in the long period and
    only 1..4 in the period of 4.  The designed cells are where the docstring of _field puts them (asserted on the restatement)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    for (Tn, rb, rows, seed) in ((T, RB, ROWS, n), (T2, RB2, ROWS2, n + 1)):
        X = _field(Tn, n, dtype, seed)
        P = len(rb) - 1
        for pad in _pads(n, dtype):
            Xd = _strided(torch, X, pad)
            for stat in ("max", "min"):
                for of in ("mean", "sum"):
                    for off in (0.0, -273.15):
                        what = (Tn, n, pad, stat, of, off)
                        got, st = engine.rolling_reduce(Xd, rb, rows, off, LENGTHS, stat=stat, of=of)
                        assert got.shape == (8, P, n) and got.dtype == tdt and int(st.item()) == 0, what
                        want = rolling_ref(X, rb, rows, off, LENGTHS, stat, of)
                        _exact(got, want, what)
                        if Tn == T:
                            assert torch.isnan(got[:, 2]).all() and torch.isnan(got[6:]).all() and not torch.isnan(got[:5, :2]).any(), what
                            assert torch.isnan(got[5, 0]).all() and not torch.isnan(got[5, 1]).any(), what
                        else:
                            assert not torch.isnan(got[:, 0]).any() and torch.isnan(got[4:, 1]).all() and not torch.isnan(got[:4, 1]).any()
    X = _field(T, n, dtype, n)
    ref = lambda W, of="sum", stat="max": rolling_ref(X, RB, ROWS, 0.0, [W], stat, of)[0].astype(np.float64)
    f64 = X.astype(np.float64)
    assert ref(1)[:2, 0].tolist() == [1000.0, 1000.0]                                      # the first entry of a list is seen
    if n > 1:
        assert ref(1)[:2, 1].tolist() == [1000.0, 1000.0]                                  # ... and the last
    if n > 2:
        assert ref(1)[0, 2] == 1000.0 and ref(2)[0, 2] == dtype(1000.0 + f64[6, 2]) < 1900.0      # rows 5 6, never 3 | 5 across the gap
    if n > 3:
        assert ref(2)[:2, 3].tolist() == [dtype(1000.0 + f64[8, 3]), dtype(1000.0 + f64[11, 3])]      # rows 8 9 | 10 11, never 9 | 10
        assert ref(1)[:2, 3].tolist() == [1000.0, 1000.0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [5, 257, 1029])
def test_nan_and_seasons(torch_cuda, dtype, n):
    """A NaN on one day of a cell rules out exactly the windows that hold it; the other cells of its 16-byte piece are as without
    it.  Season windows open all year, null (NaN everywhere), a short interval, inverted, and a day of year (row 12's) outside
    every window.  Cells 4..7 -- one 16-byte piece of an fp32 row, two of an fp64 one -- are out of season together on row 6: the
    piece is not loaded, and the windows over that day are ruled out all the same.  Whatever stands out of season (NaN, +-inf,
    1e30) is never looked at: same bits, status 0.  An all-year window for every cell gives the bits of the call without a season."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    lengths = [1, 2, 3, 5, 8]
    X = _field(T, n, dtype, seed=11 * n)
    Xn = X.copy()
    Xn[7, 1] = np.nan                                                                      # cell 1, period 0: rows 0..3 | 5 6 | 8 9 remain
    doy = np.arange(100, 100 + T)
    doy[12] = 2000
    kinds = np.array([OPEN, 1 | 0 << 10 | WIN_NULL, 102 | 107 << 10, 103 | 105 << 10 | WIN_INVERT, 300 | 320 << 10], dtype=np.int32)
    win = kinds[np.arange(n) % 5]
    win[4:8] = 106 | 106 << 10 | WIN_INVERT                                               # out on row 6 only, all four cells
    season = np.zeros((T, n), dtype=bool)
    for t in range(T):
        season[t] = in_season(int(doy[t]), win)
    assert not season[6, 4:8].any() and season[5, 4:8].all() and not season[12].any() and season[:, 0].sum() == T - 1
    poison = np.array([np.nan, np.inf, -np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 4]
    Xp = np.where(season, X, poison).astype(dtype)
    for pad in _pads(n, dtype):
        Xd, Xnd, Xpd = _strided(torch, X, pad), _strided(torch, Xn, pad), _strided(torch, Xp, pad)
        for stat, of, off in (("max", "mean", -273.15), ("min", "sum", 0.0)):
            what = (n, pad, stat, of)
            kw = dict(stat=stat, of=of)
            plain, st = engine.rolling_reduce(Xd, RB, ROWS, off, lengths, **kw)
            assert int(st.item()) == 0, what
            got, st = engine.rolling_reduce(Xnd, RB, ROWS, off, lengths, **kw)
            assert int(st.item()) == 0, what
            _exact(got, rolling_ref(Xn, RB, ROWS, off, lengths, stat, of), what)
            others = [j for j in range(n) if j != 1]
            assert torch.equal(got[:, :, others].isnan(), plain[:, :, others].isnan()), what
            assert torch.equal(got[:, :, others].nan_to_num(0.0), plain[:, :, others].nan_to_num(0.0)), what
            assert torch.isnan(got[3:, 0, 1]).all() and not torch.isnan(got[:3, 0, 1]).any() and not torch.isnan(plain[:4, 0, 1]).any()
            got, st = engine.rolling_reduce(Xd, RB, ROWS, off, lengths, doy=doy, windows=win, **kw)
            assert int(st.item()) == 0, what
            _exact(got, rolling_ref(X, RB, ROWS, off, lengths, stat, of, doy, win), what)
            assert torch.isnan(got[:, :, [j for j in range(n) if j % 5 == 1 and not 4 <= j < 8]]).all(), what      # the null windows
            g2, st = engine.rolling_reduce(Xpd, RB, ROWS, off, lengths, doy=doy, windows=win, **kw)
            assert int(st.item()) == 0 and torch.equal(g2.isnan(), got.isnan()) and torch.equal(g2.nan_to_num(0.0), got.nan_to_num(0.0)), what
            opened, _ = engine.rolling_reduce(Xd, RB, ROWS, off, lengths, doy=np.arange(100, 100 + T), windows=np.full(n, OPEN), **kw)
            assert torch.equal(opened.isnan(), plain.isnan()) and torch.equal(opened.nan_to_num(0.0), plain.nan_to_num(0.0)), what
    # the piece's cells: in season on rows 0..3, 5 | 7..9 of period 0 (row 6 is out) and rows 10 11 | 13..17 of period 1 (row 12)
    exists = ~np.isnan(rolling_ref(X, RB, ROWS, 0.0, [1, 2, 3, 4, 5], doy=doy, windows=win)[:, :, 4])
    assert exists.tolist() == [[True, True, False], [True, True, False], [True, True, False], [True, True, False], [False, True, False]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planes_rings_and_repeats(torch_cuda, dtype):
    """Plane k of an 8-window call -- unsorted, with a duplicate -- is the one-window call bit for bit; the ring does not change
    results: windows [3] alone (ring 4) = plane "3" of [3, 7] (ring 8) = plane "3" of [3, 16] (ring 16, one cell per lane); two
    runs are bit-equal.  Under a season, on both row alignments, both shapes."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    n = 257
    lengths = [7, 1, 16, 3, 9, 3, 2, 8]
    assert len(lengths) == _lib.ROLL_MAX_WINDOWS
    same = lambda a, b: torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))
    for (Tn, rb, rows) in ((T, RB, ROWS), (T2, RB2, ROWS2)):
        X = _field(Tn, n, dtype, seed=7)
        doy = np.arange(100, 100 + Tn)
        win = np.where(np.arange(n) % 3 == 0, OPEN, 101 | 130 << 10).astype(np.int32)
        for pad in _pads(n, dtype):
            Xd = _strided(torch, X, pad)
            for kw in (dict(stat="max", of="mean", doy=doy, windows=win), dict(stat="min", of="sum")):
                got, st = engine.rolling_reduce(Xd, rb, rows, -273.15, lengths, **kw)
                assert int(st.item()) == 0
                for k, W in enumerate(lengths):
                    one, _ = engine.rolling_reduce(Xd, rb, rows, -273.15, [W], **kw)
                    assert same(got[k], one[0]), (Tn, pad, k, W)
                assert same(got[3], got[5])
                again, _ = engine.rolling_reduce(Xd, rb, rows, -273.15, lengths, **kw)
                assert same(again, got)
                r4, _ = engine.rolling_reduce(Xd, rb, rows, -273.15, [3], **kw)
                r8, _ = engine.rolling_reduce(Xd, rb, rows, -273.15, [3, 7], **kw)
                r16, _ = engine.rolling_reduce(Xd, rb, rows, -273.15, [3, 16], **kw)
                assert same(r4[0], r8[0]) and same(r4[0], r16[0]) and not torch.isnan(r4[0, 0, ::3]).any()
                _exact(got, rolling_ref(X, rb, rows, -273.15, lengths, kw["stat"], kw["of"], kw.get("doy"), kw.get("windows")), (Tn, pad))
    with pytest.raises(ValueError, match="window lengths"):
        engine.rolling_reduce(Xd, RB, ROWS, 0.0, list(range(1, 10)))
    with pytest.raises(ValueError, match="window length"):
        engine.rolling_reduce(Xd, RB, ROWS, 0.0, [17])
    with pytest.raises(ValueError, match="window length"):
        engine.rolling_reduce(Xd, RB, ROWS, 0.0, [True])
    with pytest.raises(ValueError, match="stat"):
        engine.rolling_reduce(Xd, RB, ROWS, 0.0, [1], stat="mean")
    with pytest.raises(ValueError, match="go together"):
        engine.rolling_reduce(Xd, RB, ROWS, 0.0, [1], doy=np.arange(T2))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_infinity_sets_the_status_word(torch_cuda, dtype):
    """A listed, in-season +inf (or -inf) sets bit 0 and the results stay the restatement's; out of season, or in a row no list
    names (row 4, row 20), it sets nothing."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 5
    X = _field(T, n, dtype, seed=3)
    doy = np.arange(100, 100 + T)
    win = np.full(n, 100 | 110 << 10, dtype=np.int32)                                     # rows 0..10 in season
    for v in (np.inf, -np.inf):
        for t, listed, in_win in ((6, True, True), (14, True, False), (4, False, True), (20, False, False)):
            Xi = X.copy()
            Xi[t, 3] = v
            for kw in (dict(doy=doy, windows=win), {}):
                counted = listed and (in_win or not kw)
                for stat in ("max", "min"):
                    got, st = engine.rolling_reduce(torch.from_numpy(Xi).cuda(), RB, ROWS, 0.0, [1, 2, 4], stat=stat, **kw)
                    assert int(st.item()) == (1 if counted else 0), (v, t, bool(kw), stat)
                    _exact(got, rolling_ref(Xi, RB, ROWS, 0.0, [1, 2, 4], stat, "mean", kw.get("doy"), kw.get("windows")), (v, t, stat))


class _Worst:
    def __init__(self):
        self.ratio = 0.0

    def ok(self, got, want, scale, rtol, what):
        """|got - want| <= rtol * (the same aggregation of the absolute weighted parts); NaN exactly where the oracle has NaN"""
        assert got.shape == want.shape, (what, got.shape, want.shape)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        err, lim = np.abs(got[~nan].astype(np.float64) - want[~nan]), rtol * scale[~nan]
        if err.size:
            self.ratio = max(self.ratio, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), "%r: %d of %d beyond RTOL * A, worst ratio %.3g" % (what, (err > lim).sum(), err.size, self.ratio)


@pytest.mark.parametrize("dtype,kelvin", [(np.float32, True), (np.float64, False)])
def test_public_call(torch_cuda, segment_plans, dtype, kelvin):
    """tas_rolling_aggregate on a small synthetic grid with a segment table -- a Kelvin-shifted fp32 field, a plain fp64 one --
    for period="year" (40 days) and "month" (31 + 9), cells="all" and "referenced", with and without a season: against the
    restatement of the per-cell extremes aggregated by the fp64 oracle of (X W) / (1' W), within 1e-4 (fp32) / 1e-6 (fp64) of the
    same aggregation of the absolute parts (the largest ratio to that bound is printed).  Cell c.cell[1] is NaN on every third
    day: it has no window of 3 or more days in any period, so its NaN meets the contraction (it counts 0, its weight stays in the
    denominator -- the oracle's rule too).  "referenced" and "all" agree within that bound; dims, the window coordinate, the
    attributes, results_on_device(), more than 8 windows in two launches, a counted +inf raises."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, periods
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_rolling_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=29)
    Tn = c.T
    lengths = [5, 1, 3, 5, 16]
    field = c.tas.copy()
    flat = field.reshape(Tn, c.G)
    lone = int(c.cell[1])
    flat[::3, lone] = np.nan
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
            for stat, of in (("max", "mean"), ("min", "sum")):
                what = (period, season is not None, stat, of)
                cells = rolling_ref(src, rb, rows, off, lengths, stat, of).astype(np.float64)      # (n_win, P, G)
                assert np.isnan(cells[2:, :, lone]).all() and not np.isnan(cells[1, :, lone]).any() or season is not None
                want = np.stack([O.agg_coded(cells[k], c.cell, c.code, c.w_eff, c.R) for k in range(len(lengths))])
                scale = np.stack([O.agg_coded(np.abs(np.nan_to_num(cells[k], nan=0.0)), c.cell, c.code, c.w_eff, c.R) for k in range(len(lengths))])
                call = lambda d=None, **kw: tas_rolling_aggregate(d if d is not None else ds(), lengths, "popwt", "reg", c.df, stat=stat, of=of,
                                                                  period=period, season=season, **kw)
                out = call()
                v = out["tas-rolling"]
                assert v.dims == ("window", "period", "reg") and v.attrs["stat"] == stat and v.attrs["of"] == of, what
                assert v.attrs.get("units") == ("C" if kelvin else None)
                assert out["window"].values.dtype == np.int64 and list(out["window"].values) == lengths
                assert len(out["period"].values) == P
                got = v.values
                assert isinstance(v.data, np.ndarray) and got.dtype == dtype and got.shape == (len(lengths), P, c.R)
                assert np.isnan(got[:, :, c.R - 1]).all()                                 # the region without weight
                worst.ok(got, want, scale, c.rtol, what)
                np.testing.assert_array_equal(got[0], got[3])                             # the duplicate window
                ref = call(cells="referenced")["tas-rolling"].values
                worst.ok(ref, want, scale, c.rtol, what + ("referenced",))
                worst.ok(ref, got.astype(np.float64), scale, c.rtol, what + ("referenced vs all",))
                np.testing.assert_array_equal(call(ds(device=False))["tas-rolling"].values, got)
    print("rolling public call %s: largest |got - ref| / (RTOL * A) = %.3g" % (np.dtype(dtype).name, worst.ratio))
    with pkg.results_on_device():
        on = call()
        assert isinstance(on["tas-rolling"].data, torch.Tensor) and on["tas-rolling"].data.is_cuda
        assert isinstance(call(ds(device=False))["tas-rolling"].data, np.ndarray)
    np.testing.assert_array_equal(on["tas-rolling"].values, got)
    other = call(varname="coldest")
    np.testing.assert_array_equal(other["coldest"].values, got)
    # more than 8 windows: 8, then 2, joined in the caller's order
    ran = []
    real = engine.rolling_reduce
    ten = list(range(10, 0, -1))
    many = lambda w: tas_rolling_aggregate(ds(), w, "popwt", "reg", c.df, period="month")["tas-rolling"].values
    try:
        engine.rolling_reduce = lambda *a, **k: (ran.append(len(a[4])), real(*a, **k))[1]
        v10 = many(ten)
    finally:
        engine.rolling_reduce = real
    assert ran == [8, 2] and v10.shape == (10, 2, c.R)
    np.testing.assert_array_equal(v10[:8], many(ten[:8]))
    np.testing.assert_array_equal(v10[8:], many(ten[8:]))
    # a counted +inf raises
    hit = field.copy()
    hit.reshape(Tn, c.G)[3, int(c.cell[0])] = np.inf
    for cells_kw in ("all", "referenced"):
        with pytest.raises(ValueError, match="inf"):
            tas_rolling_aggregate(ds(f=hit), [1, 3], "popwt", "reg", c.df, period="year", cells=cells_kw)
