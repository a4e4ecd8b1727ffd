"""Spell statistics on the GPU (run with -m gpu): wagg_spell_reduce_* through engine.spell_reduce against the NumPy restatement
tests/spell_ref.py, and tas_spell_aggregate on a segment table against that restatement aggregated by the fp64 oracle.

Counts are integers: they are compared EXACTLY, never by tolerance; only the weighted mean of the public call rounds.
The kernel cases share one shape: T = 23 rows, three periods whose lists hold 9, 8 and 0 entries -- rows 0..9 without row 4 (a
gap inside the first period), rows 10..17, nothing -- so that rows 9 | 10 are consecutive across a period boundary."""
import numpy as np
import pytest

from tests.spell_ref import WIN_INVERT, WIN_NULL, in_season, spell_ref
from tests.test_gpu_packed_totals import _Sparse, segment_plans  # noqa: F401
from tests.test_gpu_parity import _rel_ok

pytestmark = pytest.mark.gpu

T = 23
RB = np.array([0, 9, 17, 17])
ROWS = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17])
LISTS = (9, 8, 0)
NS = (1, 3, 4, 5, 257, 1029)
OPEN = 0 | 1023 << 10
STATS = ("days", "events", "longest")
SIDES = ("above", "below")


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


def _field(n, dtype, seed):
    """Values in 0..10 (thresholds lie between them).  Cell 0 is 9 throughout: its run starts on a list's first entry, ends on its
    last, and straddles the gap and the period boundary; cells 1.. carry runs that start on every entry of the first list, odd
    and even, of lengths 2 and 3; the rest is random with long and short runs."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 10.0, (T, n))
    long_runs = rng.uniform(size=n) < 0.5
    X[:, long_runs] = np.where(rng.uniform(size=(T, int(long_runs.sum()))) < 0.85, 8.5, 1.5)
    for j in range(min(n, 40)):
        if j == 0:
            X[:, j] = 9.0
        else:
            X[:, j] = 1.0
            start, length = (j - 1) % 10, 2 + (j - 1) // 10 % 2        # rows start .. start + length - 1
            X[start:start + length, j] = 9.0
            X[start + 11:start + 11 + length, j] = 9.0                   # ... and the same in the second period
    return X.astype(dtype)


def _exact(got, want, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%r: %d counts differ, first at (threshold, period, cell) %r: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_counts_equal_the_restatement(torch_cuda, dtype, n):
    """All three statistics, both sides, min_length 1, 2, the list's length and one more, on aligned rows (a partial last piece
    for n = 1, 3, 5, 257, 1029; more than one column block for 1029) and on rows that are not 16-byte aligned; no season.
    The designed cells' runs are where the docstring of _field puts them (checked on the restatement)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    X = _field(n, dtype, seed=n)
    thr = [5.0, 2.0, 8.75]
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    for pad in _pads(n, dtype):
        Xd = _strided(torch, X, pad)
        for side in SIDES:
            for stat in STATS:
                for L in ((1,) if stat == "longest" else (1, 2, LISTS[0], LISTS[0] + 1)):
                    what = (n, pad, side, stat, L)
                    got, st = engine.spell_reduce(Xd, RB, ROWS, 0.0, thr, min_length=L, stat=stat, side=side)
                    assert got.shape == (3, 3, n) and got.dtype == tdt and int(st.item()) == 0, what
                    _exact(got, spell_ref(X, RB, ROWS, 0.0, thr, L, stat, side), what)
                    assert (got[:, 2] == 0).all(), what                                   # the empty period
    want = lambda stat, L: spell_ref(X, RB, ROWS, 0.0, [5.0], L, stat)[0]
    # cell 0: nine hot entries cut by the gap into 4 + 5; eight in the second period (never 9 + 8 = 17 in one run)
    assert want("longest", 1)[:, 0].tolist() == [5, 8, 0] and want("events", 1)[:, 0].tolist() == [2, 1, 0]
    assert want("days", LISTS[0])[:, 0].tolist() == [0, 0, 0] and want("days", 5)[:, 0].tolist() == [5, 8, 0]
    if n > 5:
        assert want("days", 2)[0, 3] == 2 and want("days", 2)[0, 4] == 0                   # rows 2 3 | row 3 and the dropped row 4
        assert want("longest", 1)[:, 10].tolist() == [1, 1, 0]                            # rows 9 10: cut by the period boundary


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_threshold_counts_and_planes(torch_cuda, dtype):
    """1, G, G + 1 and 64 thresholds (a ragged last group), unsorted with a duplicate, under a season: plane k of the
    many-threshold call is the one-threshold call bit for bit, and the restatement's; two runs are bit-equal."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    n, G = 257, _lib.SPELL_GROUP
    X = _field(n, dtype, seed=7)
    doy = np.arange(100, 100 + T)
    win = np.where(np.arange(n) % 3 == 0, OPEN, 101 | 112 << 10).astype(np.int32)
    rng = np.random.default_rng(3)
    thr64 = rng.permutation(np.linspace(0.5, 9.5, 64))
    thr64[17] = thr64[40]                                                                 # a duplicate
    kw = dict(doy=doy, windows=win, min_length=2)
    for pad in _pads(n, dtype):
        Xd = _strided(torch, X, pad)
        for stat, side in (("days", "above"), ("events", "below")):
            ones = [engine.spell_reduce(Xd, RB, ROWS, 0.0, [t], stat=stat, side=side, **kw)[0] for t in thr64]
            for count in (1, G, G + 1, 64):
                got, st = engine.spell_reduce(Xd, RB, ROWS, 0.0, thr64[:count], stat=stat, side=side, **kw)
                assert got.shape == (count, 3, n) and int(st.item()) == 0
                for k in range(count):
                    assert torch.equal(got[k], ones[k][0]), (pad, stat, count, k)
                _exact(got, spell_ref(X, RB, ROWS, 0.0, thr64[:count], 2, stat, side, doy, win), (pad, stat, count))
            again, _ = engine.spell_reduce(Xd, RB, ROWS, 0.0, thr64, stat=stat, side=side, **kw)
            assert torch.equal(again, got) and torch.equal(got[17], got[40])
    with pytest.raises(ValueError, match="thresholds"):
        engine.spell_reduce(Xd, RB, ROWS, 0.0, list(range(_lib.SPELL_MAX + 1)))
    with pytest.raises(ValueError, match="thresholds"):
        engine.spell_reduce(Xd, RB, ROWS, 0.0, [1.0, float("inf")])
    with pytest.raises(ValueError, match="min_length"):
        engine.spell_reduce(Xd, RB, ROWS, 0.0, [1.0], min_length=0)
    with pytest.raises(ValueError, match="longest"):
        engine.spell_reduce(Xd, RB, ROWS, 0.0, [1.0], min_length=2, stat="longest")
    with pytest.raises(ValueError, match="go together"):
        engine.spell_reduce(Xd, RB, ROWS, 0.0, [1.0], doy=doy)


def test_fp32_kelvin_field_is_classified_as_in_fp64(torch_cuda):
    """35 C on a Kelvin field: 35 + 273.15 is no float32.  Values one ulp below, on and one ulp above float32(308.15), in runs:
    the counts are those of the fp64 classification float64(x) - 273.15 >= 35 -- on both sides, where a shift in fp32 would
    move the values on the threshold's rounding."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    thr, off = 35.0, -273.15
    c = thr - off
    f = np.float32(c)
    assert float(f) != c                                                                  # the fp64 shift is not representable
    lo, hi = np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1e9))
    vals = np.array([lo, f, hi], dtype=np.float32)
    hot64 = vals.astype(np.float64) + off >= thr
    assert hot64.tolist() == [v >= c for v in vals.astype(np.float64)] and hot64[2] and not hot64[0]
    n = 27 * 5
    X = np.empty((T, n), dtype=np.float32)
    for j in range(n):                                                                    # every triple of the three values, repeating
        X[:, j] = vals[[(j // 3 ** (t % 3)) % 3 for t in range(T)]]
    X[:, 27:54] = np.roll(X[:, 27:54], 1, axis=0)
    for pad in _pads(n, np.float32):
        Xd = _strided(torch, X, pad)
        for side in SIDES:
            for stat, L in (("days", 1), ("days", 2), ("events", 2), ("longest", 1)):
                got, st = engine.spell_reduce(Xd, RB, ROWS, off, [thr], min_length=L, stat=stat, side=side)
                assert int(st.item()) == 0
                _exact(got, spell_ref(X, RB, ROWS, off, [thr], L, stat, side), (pad, side, stat, L))
    Xc = np.tile(vals[:, None], (1, 4))                                                   # one value per row, one row per period
    one, _ = engine.spell_reduce(torch.from_numpy(Xc).cuda(), [0, 1, 2, 3], [0, 1, 2], off, [thr])
    assert one[0, :, 0].tolist() == [float(h) for h in hot64]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [5, 257, 1029])
def test_seasons(torch_cuda, dtype, n):
    """Windows open all year, null, ordinary, inverted, and a day of year (row 12's) outside every window: an out-of-season day
    inside a run cuts it.  Cells 4..7 -- one 16-byte piece of an fp32 row, two of an fp64 one -- are out of season together on
    row 6: the piece is not loaded, and the runs are reset all the same.  Whatever stands out of season (NaN, +-inf, 1e30) is
    never looked at: same counts, status 0.  An all-year window for every cell gives the bits of the call without a season."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    X = _field(n, dtype, seed=11 * n)
    X[:, 4:8] = 9.0
    doy = np.arange(100, 100 + T)
    doy[12] = 2000
    kinds = np.array([OPEN, 1 | 0 << 10 | WIN_NULL, 102 | 107 << 10, 103 | 105 << 10 | WIN_INVERT, 300 | 320 << 10], dtype=np.int32)
    win = kinds[np.arange(n) % 5]
    win[4:8] = 106 | 106 << 10 | WIN_INVERT                                               # out on row 6 only, all four cells
    thr = [5.0, 8.75]
    season = np.zeros((T, n), dtype=bool)
    for t in range(T):
        season[t] = in_season(int(doy[t]), win)
    assert not season[6, 4:8].any() and season[5, 4:8].all() and not season[12].any() and season[:, 0].sum() == T - 1
    poison = np.array([np.nan, np.inf, -np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 4]
    Xp = np.where(season, X, poison).astype(dtype)
    for pad in _pads(n, dtype):
        Xd, Xpd = _strided(torch, X, pad), _strided(torch, Xp, pad)
        for side in SIDES:
            for stat, L in (("days", 1), ("days", 3), ("events", 2), ("longest", 1)):
                what = (n, pad, side, stat, L)
                kw = dict(min_length=L, stat=stat, side=side)
                got, st = engine.spell_reduce(Xd, RB, ROWS, 0.0, thr, doy=doy, windows=win, **kw)
                assert int(st.item()) == 0, what
                want = spell_ref(X, RB, ROWS, 0.0, thr, L, stat, side, doy, win)
                _exact(got, want, what)
                g2, st = engine.spell_reduce(Xpd, RB, ROWS, 0.0, thr, doy=doy, windows=win, **kw)
                assert torch.equal(g2, got) and int(st.item()) == 0, what
                plain, _ = engine.spell_reduce(Xd, RB, ROWS, 0.0, thr, **kw)
                opened, _ = engine.spell_reduce(Xd, RB, ROWS, 0.0, thr, doy=np.arange(100, 100 + T), windows=np.full(n, OPEN), **kw)
                assert torch.equal(opened, plain), what
    # the piece's cells: hot on all of rows 0..9 but row 4 (the gap) and row 6 (out of season): runs 0-3, 5, 7-9 | 10 11, 13-17
    longest = spell_ref(X, RB, ROWS, 0.0, [5.0], 1, "longest", "above", doy, win)[0]
    events = spell_ref(X, RB, ROWS, 0.0, [5.0], 1, "events", "above", doy, win)[0]
    assert longest[:, 4].tolist() == [4, 5, 0] and events[:, 4].tolist() == [3, 2, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(torch_cuda, dtype):
    """NaN cuts a run and sets no status.  An in-season +-inf sets bit 0 whether it is hot or not (+inf below a threshold is
    cold); the counts stay the restatement's.  Out of season it sets nothing."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 5
    X = np.full((T, n), 9.0, dtype=dtype)
    X[2, 1] = np.nan
    got, st = engine.spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, [5.0], stat="events")
    assert int(st.item()) == 0 and got[0, :, 1].tolist() == [3, 1, 0] and got[0, :, 0].tolist() == [2, 1, 0]   # rows 0 1 | 3 | 5..9
    got, st = engine.spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, [5.0], stat="longest", side="below")
    assert int(st.item()) == 0 and (got == 0).all()
    doy = np.arange(100, 100 + T)
    win = np.full(n, 100 | 110 << 10, dtype=np.int32)                                     # rows 0..10 in season
    for v in (np.inf, -np.inf):
        for side in SIDES:
            for t, counted in ((6, True), (14, False)):
                Xi = X.copy()
                Xi[t, 3] = v
                for kw in (dict(doy=doy, windows=win), {}):
                    is_counted = counted or not kw
                    got, st = engine.spell_reduce(torch.from_numpy(Xi).cuda(), RB, ROWS, 0.0, [5.0], min_length=2, side=side, **kw)
                    assert int(st.item()) == (1 if is_counted else 0), (v, side, t, bool(kw))
                    _exact(got, spell_ref(Xi, RB, ROWS, 0.0, [5.0], 2, "days", side, kw.get("doy"), kw.get("windows")), (v, side, t))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cross_family_laws(torch_cuda, dtype):
    """days with min_length 1 above a threshold = the bins' count of [thr, +inf), bit for bit, on a finite field, with and
    without a season; days >= min_length * events and longest <= the list's length everywhere; events with min_length 1 >=
    events with min_length 2; days is monotone in min_length."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 1029
    X = (_field(n, dtype, seed=5) + dtype(273.15)).astype(dtype)
    thr = [5.0, 2.0, 8.75, 5.0]
    doy = np.arange(100, 100 + T)
    win = np.where(np.arange(n) % 4 == 1, 103 | 109 << 10, OPEN).astype(np.int32)
    for pad in _pads(n, dtype):
        Xd = _strided(torch, X, pad)
        for kw in ({}, dict(doy=doy, windows=win)):
            days1, _ = engine.spell_reduce(Xd, RB, ROWS, -273.15, thr, min_length=1, **kw)
            for k, t in enumerate(thr):
                bins, _ = engine.bin_days_reduce(Xd, RB, ROWS, -273.15, [t, float("inf")], **kw)
                assert torch.equal(days1[k], bins[0]), (pad, k)
            longest, _ = engine.spell_reduce(Xd, RB, ROWS, -273.15, thr, stat="longest", **kw)
            prev_days, prev_events = days1, None
            for L in (1, 2, 3, 9):
                days, _ = engine.spell_reduce(Xd, RB, ROWS, -273.15, thr, min_length=L, **kw)
                events, _ = engine.spell_reduce(Xd, RB, ROWS, -273.15, thr, min_length=L, stat="events", **kw)
                assert (days >= L * events).all() and (days <= prev_days).all()
                assert prev_events is None or (events <= prev_events).all()
                assert ((events > 0) == (longest >= L)).all() and ((days > 0) == (longest >= L)).all()
                prev_days, prev_events = days, events
            for p, length in enumerate(LISTS):
                assert (longest[:, p] <= length).all() and (days1[:, p] <= length).all()
            assert (longest <= days1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_public_call(torch_cuda, segment_plans, dtype):
    """tas_spell_aggregate on a small synthetic grid with a segment table, a Kelvin-shifted field and period="month" (31 days,
    then 9): every statistic against the restatement of the per-cell counts aggregated by the fp64 oracle of (X W) / (1' W), at
    the project's 1e-4 (fp32) / 1e-6 (fp64) -- only the weighted mean rounds; cells="all" and "referenced", device- and
    host-resident; dims, the threshold coordinate, the attributes, results_on_device(); an in-season +-inf raises."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_spell_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=29)
    Tn = c.T
    rb, rows = np.array([0, 31, Tn]), np.arange(Tn)
    thr = [10.0, 0.0, 10.0, 21.5]
    flat = c.tas.reshape(Tn, c.G)
    ds = lambda device=True, f=None: convert_kelvin_to_celsius(c.dataset(torch, device=device, tas=c.tas if f is None else f), "tas")
    call = lambda d=None, **kw: tas_spell_aggregate(d if d is not None else ds(), thr, "popwt", "reg", c.df, period="month", **kw)
    for stat, side, L in (("days", "above", 3), ("events", "above", 2), ("longest", "below", 3), ("days", "below", 1)):
        kw = dict(stat=stat, side=side, min_length=L)
        eff = 1 if stat == "longest" else L
        cells = spell_ref(flat, rb, rows, -273.15, thr, eff, stat, side)                   # (n_thr, P, G)
        assert cells.max() >= eff and len(np.unique(cells)) > 2
        want = np.stack([O.agg_coded(cells[k], c.cell, c.code, c.w_eff, c.R) for k in range(len(thr))])
        out = call(**kw)
        v = out["tas-spell"]
        assert v.dims == ("threshold", "period", "reg") and v.attrs["units"] == ("1" if stat == "events" else "days")
        assert v.attrs["min_length"] == eff and v.attrs["stat"] == stat and v.attrs["side"] == side
        assert out["threshold"].values.dtype == np.float64 and list(out["threshold"].values) == thr
        assert len(out["period"].values) == 2
        got = v.values
        assert isinstance(v.data, np.ndarray) and got.dtype == dtype and got.shape == (len(thr), 2, c.R)
        assert np.isnan(got[:, :, c.R - 1]).all()                                         # the region without weight
        _rel_ok(got, want, c.rtol)
        np.testing.assert_array_equal(got[0], got[2])                                     # the duplicate threshold
        ref = call(cells="referenced", **kw)["tas-spell"].values
        _rel_ok(ref, want, c.rtol)
        np.testing.assert_array_equal(call(ds(device=False), **kw)["tas-spell"].values, got)
        np.testing.assert_array_equal(call(ds(device=False), cells="referenced", **kw)["tas-spell"].values, ref)
    with pkg.results_on_device():
        on = call(**kw)
        assert isinstance(on["tas-spell"].data, torch.Tensor) and on["tas-spell"].data.is_cuda
        assert isinstance(call(ds(device=False), **kw)["tas-spell"].data, np.ndarray)
    np.testing.assert_array_equal(on["tas-spell"].values, got)
    other = call(varname="cold-days", **kw)
    np.testing.assert_array_equal(other["cold-days"].values, got)
    # a counted +-inf raises, hot or not; in a quad no row reads it is nobody's business for cells="referenced"
    in_row = c.plan().compact_cells(dtype)
    poisoned = c.poisoned(c.tas, in_row)
    np.testing.assert_array_equal(call(ds(f=poisoned), cells="referenced", **kw)["tas-spell"].values, ref)
    with pytest.raises(ValueError, match="inf"):
        call(ds(f=poisoned), **kw)
    hit = c.tas.copy()
    hit.reshape(Tn, c.G)[3, int(c.cell[0])] = np.inf
    for cells_kw in ("all", "referenced"):
        with pytest.raises(ValueError, match="inf"):
            call(ds(f=hit), cells=cells_kw, stat="days", side="below")


def test_more_than_64_thresholds_run_in_two_launches(torch_cuda, segment_plans, monkeypatch):
    """70 thresholds: 64, then 6, joined in the caller's order"""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.transformations import tas_spell_aggregate
    torch = torch_cuda
    c = _Sparse(16, 32, np.float32, seed=31)
    thr = list(np.linspace(300.0, 260.0, 70))
    ran = []
    real = engine.spell_reduce
    monkeypatch.setattr(engine, "spell_reduce", lambda *a, **k: (ran.append(len(a[4])), real(*a, **k))[1])
    call = lambda t: tas_spell_aggregate(c.dataset(torch), t, "popwt", "reg", c.df, min_length=2, period="year")["tas-spell"].values
    v = call(thr)
    assert ran == [64, 6] and v.shape == (70, 1, c.R)
    np.testing.assert_array_equal(v[:64], call(thr[:64]))
    np.testing.assert_array_equal(v[64:], call(thr[64:]))
