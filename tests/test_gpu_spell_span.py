"""Spells that run across period boundaries on the GPU (run with -m gpu): wagg_spell_span_* through
engine.spell_reduce(span="record") against the NumPy restatement tests/spell_span_ref.py, and tas_spell_aggregate(span="record")
on a segment table against that restatement aggregated by the fp64 oracle.

Counts are integers: they are compared EXACTLY, never by tolerance; only the weighted mean of the public call rounds.  The
kernel cases share T = 26 rows and five sets of lists (LISTS below): the 9, 8, 0 shape of tests/test_gpu_spell.py, whose rows 9 |
10 join across the boundary; 4, 1, 0, 5 and 1, 1, 1, 1, 6, whose lists are shorter than min_length, so that a credit of days
crosses several lists and an empty one; a row gap exactly at a boundary; and out-of-range row indices as a list's last entry.
Fields take their values from {1.5, 4, 6.5, 8.5, 9.5}, between the thresholds: cell 0 is hot throughout, the cells behind it
carry one run each that starts and ends on every entry around each boundary, the rest are hot with probability 0.85, so that
most of their runs cross."""
import ctypes as C

import numpy as np
import pytest

from tests import rowlist_layout as RL
from tests.spell_ref import WIN_INVERT, WIN_NULL, in_season, spell_ref
from tests.spell_span_ref import running_and_whole, spell_span_ref, stats_from
from tests.test_gpu_packed_totals import _Sparse, segment_plans  # noqa: F401
from tests.test_gpu_parity import _rel_ok
from tests.test_gpu_spell import OPEN, _exact, _pads, _strided

pytestmark = pytest.mark.gpu

T = 26
LISTS = {
    "9-8-0": (np.array([0, 9, 17, 17]), np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17])),
    "4-1-0-5": (np.array([0, 4, 5, 5, 10]), np.arange(10)),
    "1-1-1-1-6": (np.array([0, 1, 2, 3, 4, 10]), np.arange(10)),
    "gap": (np.array([0, 6, 12]), np.array([0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12])),
    # a row behind the field, then the row that would follow it were it inside; -1, then row 0; the last list goes on from row 7
    "outside": (np.array([0, 5, 9, 13, 17]), np.array([3, 4, 5, 6, T, T + 1, 0, 1, -1, 0, 1, 2, 3, 4, 5, 6, 7])),
}
NS = (1, 3, 4, 5, 257, 1029)
THR9 = [5.0, 2.0, 8.75, 7.0, 9.0, 3.0, 5.0, 1.0, 9.75]      # a full group and a ragged second one; a duplicate; none hot above 9.75
STATS = ("days", "events", "longest")
SIDES = ("above", "below")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _field(n, dtype, seed, nan=True):
    rng = np.random.default_rng(seed)
    X = np.where(rng.uniform(size=(T, n)) < 0.85, rng.choice([8.5, 9.5], (T, n)), rng.choice([1.5, 4.0, 6.5], (T, n)))
    X[:, 0] = 9.5
    runs = [(s, e) for b in (4, 5, 6, 9, 10, 13, 17) for s in (b - 2, b - 1, b) for e in (b - 1, b, b + 1) if s <= e]
    for j, (s, e) in enumerate(runs, start=1):               # one run per cell, rows s .. e, around every boundary of every set
        if j < n:
            X[:, j] = 1.5
            X[s:e + 1, j] = 9.5
    if nan and n > 200:                                      # a NaN on either side of a boundary, in cells that are hot otherwise
        for j, t in ((100, 8), (101, 9), (102, 10), (103, 3), (104, 4), (105, 5), (106, 12), (107, 13)):
            X[:, j] = 8.5
            X[t, j] = np.nan
    return X.astype(dtype)


def _lists_dev(torch, name):
    rb, rows = LISTS[name]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    return i32(rb), i32(rows)                                # (handed over with checked=True: "outside" would not pass the check)


def _chain_len(name):
    return int(LISTS[name][0][-1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_counts_equal_the_restatement(torch_cuda, dtype, n):
    """Every set of lists, both sides, days and events with min_length 1, 2, 3, 6 and one more than the chain's length, longest;
    nine thresholds; rows that keep and that break 16-byte alignment; a partial last piece (n = 1, 3, 5, 257, 1029), a second
    column block (1029).  The empty periods are 0, a second call into the same ``out`` gives the same bits."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    X = _field(n, dtype, seed=n)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    devs = [(pad, _strided(torch, X, pad)) for pad in _pads(n, dtype)]
    crossed = 0
    for name, (rb, rows) in LISTS.items():
        rbd, rwd = _lists_dev(torch, name)
        P = len(rb) - 1
        for side in SIDES:
            period_of, r, ell = running_and_whole(X, rb, rows, 0.0, THR9, side)
            for stat in STATS:
                for L in ((1,) if stat == "longest" else (1, 2, 3, 6, _chain_len(name) + 1)):
                    want = stats_from(period_of, r, ell, P, L, stat)
                    crossed += int((want != spell_ref(X, rb, rows, 0.0, THR9, L, stat, side)).any())
                    for pad, Xd in devs:
                        what = (name, n, pad, side, stat, L)
                        got, st = engine.spell_reduce(Xd, rbd, rwd, 0.0, THR9, min_length=L, stat=stat, side=side, checked=True, span="record")
                        assert got.shape == (9, P, n) and got.dtype == tdt and int(st.item()) == 0, what
                        _exact(got, want, what)
                    if L == 6 or stat == "longest":
                        keep = got.clone()
                        again, _ = engine.spell_reduce(Xd, rbd, rwd, 0.0, THR9, min_length=L, stat=stat, side=side, checked=True, out=got,
                                                       span="record")
                        assert again is got and torch.equal(again, keep), what
    assert crossed >= 10                                     # the span mode differs from the truncating one in most cases
    # the all-hot cell: the issue's hand-worked case and its neighbours
    rb, rows = LISTS["4-1-0-5"]
    one = lambda stat, L: spell_span_ref(X[:, :1], rb, rows, 0.0, [5.0], L, stat)[0, :, 0].tolist()
    assert one("days", 6) == [4, 1, 0, 5] and one("events", 6) == [0, 0, 0, 1] and one("longest", 1) == [4, 5, 0, 10]
    rb, rows = LISTS["1-1-1-1-6"]
    one = lambda stat, L: spell_span_ref(X[:, :1], rb, rows, 0.0, [5.0], L, stat)[0, :, 0].tolist()
    assert one("days", 6) == [1, 1, 1, 1, 6] and one("events", 6) == [0, 0, 0, 0, 1] and one("events", 3) == [0, 0, 1, 0, 0]
    rb, rows = LISTS["gap"]
    assert spell_span_ref(X[:, :1], rb, rows, 0.0, [5.0], 1, "longest")[0, :, 0].tolist() == [6, 6]
    rb, rows = LISTS["outside"]
    assert spell_span_ref(X[:, :1], rb, rows, 0.0, [5.0], 1, "longest")[0, :, 0].tolist() == [4, 2, 4, 8]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_threshold_counts_and_planes(torch_cuda, dtype):
    """1, 8 and 9 thresholds: plane k of the many-threshold call is the one-threshold call bit for bit, and the restatement's"""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 257
    X = _field(n, dtype, seed=7)
    for name in ("9-8-0", "1-1-1-1-6"):
        rb, rows = LISTS[name]
        rbd, rwd = _lists_dev(torch, name)
        for pad in _pads(n, dtype):
            Xd = _strided(torch, X, pad)
            for stat, side, L in (("days", "above", 6), ("events", "below", 2), ("longest", "above", 1)):
                kw = dict(min_length=L, stat=stat, side=side, checked=True, span="record")
                ones = [engine.spell_reduce(Xd, rbd, rwd, 0.0, [t], **kw)[0] for t in THR9]
                for count in (1, 8, 9):
                    got, st = engine.spell_reduce(Xd, rbd, rwd, 0.0, THR9[:count], **kw)
                    assert got.shape == (count, len(rb) - 1, n) and int(st.item()) == 0
                    for k in range(count):
                        assert torch.equal(got[k], ones[k][0]), (name, pad, stat, count, k)
                    _exact(got, spell_span_ref(X, rb, rows, 0.0, THR9[:count], L, stat, side), (name, pad, stat, count))
                assert torch.equal(got[0], got[6])           # the duplicate threshold


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [5, 257, 1029])
def test_seasons(torch_cuda, dtype, n):
    """Windows open all year, null, ordinary and inverted; a window that closes on the last day of a period (its run must not
    go on); cells 4..7 -- one 16-byte piece of an fp32 row, two of an fp64 one -- out of season together on the FIRST entry of
    the second list: the piece is not loaded and the runs are reset all the same.  Whatever stands out of season is never
    looked at; an all-year window for every cell gives the bits of the call without a season."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    X = _field(n, dtype, seed=11 * n, nan=False)
    X[:, 4:8] = 9.5
    doy = np.arange(100, 100 + T)
    for name, first_of_second, last_of_first in (("9-8-0", 10, 9), ("4-1-0-5", 4, 3), ("gap", 7, 5)):
        rb, rows = LISTS[name]
        rbd, rwd = _lists_dev(torch, name)
        kinds = np.array([OPEN, 1 | 0 << 10 | WIN_NULL, 100 | (100 + last_of_first) << 10, 103 | 105 << 10 | WIN_INVERT,
                          (100 + first_of_second) | 125 << 10], dtype=np.int32)
        win = kinds[np.arange(n) % 5]
        d1 = 100 + first_of_second
        win[4:8] = d1 | d1 << 10 | WIN_INVERT                # out on the first entry of the second list only, all four cells
        season = np.stack([in_season(int(d), win) for d in doy])
        assert not season[first_of_second, 4:8].any() and season[last_of_first, 4:8].all()
        poison = np.array([np.nan, np.inf, -np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 4]
        Xp = np.where(season, X, poison).astype(dtype)
        thr = [5.0, 8.75]
        for pad in _pads(n, dtype):
            Xd, Xpd = _strided(torch, X, pad), _strided(torch, Xp, pad)
            for side in SIDES:
                for stat, L in (("days", 1), ("days", 3), ("days", 6), ("events", 2), ("longest", 1)):
                    what = (name, n, pad, side, stat, L)
                    kw = dict(min_length=L, stat=stat, side=side, checked=True, span="record")
                    got, st = engine.spell_reduce(Xd, rbd, rwd, 0.0, thr, doy=doy, windows=win, **kw)
                    assert int(st.item()) == 0, what
                    _exact(got, spell_span_ref(X, rb, rows, 0.0, thr, L, stat, side, doy, win), what)
                    g2, st = engine.spell_reduce(Xpd, rbd, rwd, 0.0, thr, doy=doy, windows=win, **kw)
                    assert torch.equal(g2, got) and int(st.item()) == 0, what
                    plain, _ = engine.spell_reduce(Xd, rbd, rwd, 0.0, thr, **kw)
                    opened, _ = engine.spell_reduce(Xd, rbd, rwd, 0.0, thr, doy=doy, windows=np.full(n, OPEN), **kw)
                    assert torch.equal(opened, plain), what
        # the piece's cells: hot throughout, cut on the first entry of the second list alone
        longest = spell_span_ref(X, rb, rows, 0.0, [5.0], 1, "longest", "above", doy, win)[0]
        if name == "4-1-0-5":
            assert longest[:, 4].tolist() == [4, 0, 0, 5]
        if name == "9-8-0":
            assert longest[:, 4].tolist() == [5, 7, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(torch_cuda, dtype):
    """NaN on either side of a boundary cuts the run and sets no status.  An in-season +-inf sets bit 0 whether it is hot or not;
    the counts stay the restatement's.  Out of season it sets nothing."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 5
    rb, rows = LISTS["9-8-0"]
    rbd, rwd = _lists_dev(torch, "9-8-0")
    X = np.full((T, n), 9.0, dtype=dtype)
    X[9, 1] = np.nan                                         # the last entry of the first list
    X[10, 2] = np.nan                                        # the first entry of the second
    got, st = engine.spell_reduce(torch.from_numpy(X).cuda(), rbd, rwd, 0.0, [5.0], stat="longest", checked=True, span="record")
    assert int(st.item()) == 0
    assert got[0, :, 0].tolist() == [5, 13, 0] and got[0, :, 1].tolist() == [4, 8, 0] and got[0, :, 2].tolist() == [5, 7, 0]
    doy = np.arange(100, 100 + T)
    win = np.full(n, 100 | 110 << 10, dtype=np.int32)        # rows 0..10 in season
    for v in (np.inf, -np.inf):
        for side in SIDES:
            for t, counted in ((9, True), (14, False)):
                Xi = X.copy()
                Xi[t, 3] = v
                for kw in (dict(doy=doy, windows=win), {}):
                    is_counted = counted or not kw
                    got, st = engine.spell_reduce(torch.from_numpy(Xi).cuda(), rbd, rwd, 0.0, [5.0], min_length=6, side=side, checked=True,
                                                  span="record", **kw)
                    assert int(st.item()) == (1 if is_counted else 0), (v, side, t, bool(kw))
                    _exact(got, spell_span_ref(Xi, rb, rows, 0.0, [5.0], 6, "days", side, kw.get("doy"), kw.get("windows")), (v, side, t))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_where_nothing_crosses_the_result_is_the_truncating_call_bit_for_bit(torch_cuda, dtype):
    """A cold day on the first entry of every list behind the first: span="record" equals span="period" in its bits, for every
    statistic; and on the unchanged field LONGEST is never below the truncating value, the sums over the periods are those of
    the chain as one list."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = 1029
    X = _field(n, dtype, seed=5)
    for name in ("9-8-0", "4-1-0-5", "gap"):
        rb, rows = LISTS[name]
        rbd, rwd = _lists_dev(torch, name)
        one = torch.tensor([0, len(rows)], dtype=torch.int32, device="cuda")
        Xc = X.copy()
        for p in range(1, len(rb) - 1):
            if rb[p] < rb[-1]:
                Xc[rows[rb[p]]] = 4.0
        for pad in _pads(n, dtype):
            Xd, Xcd = _strided(torch, X, pad), _strided(torch, Xc, pad)
            for stat, L in (("days", 1), ("days", 3), ("days", 6), ("events", 2), ("longest", 1)):
                kw = dict(min_length=L, stat=stat, checked=True)
                a, _ = engine.spell_reduce(Xcd, rbd, rwd, 0.0, [5.0, 9.0], span="record", **kw)
                b, _ = engine.spell_reduce(Xcd, rbd, rwd, 0.0, [5.0, 9.0], span="period", **kw)
                assert torch.equal(a, b), (name, pad, stat, L)
                rec, _ = engine.spell_reduce(Xd, rbd, rwd, 0.0, [5.0, 9.0], span="record", **kw)
                cut, _ = engine.spell_reduce(Xd, rbd, rwd, 0.0, [5.0, 9.0], **kw)
                whole, _ = engine.spell_reduce(Xd, one, rwd, 0.0, [5.0, 9.0], **kw)
                if stat == "longest":
                    assert torch.equal(rec.max(dim=1).values, whole[:, 0]) and (rec >= cut).all(), (name, pad)
                else:
                    assert torch.equal(rec.sum(dim=1), whole[:, 0]), (name, pad, stat, L)


@pytest.mark.parametrize("dtype", RL.DTYPES)
def test_pitched_and_poisoned_out(torch_cuda, dtype):
    """The C entry point with ldo = n + 5, out_pstride = P * ldo + 7 at a base one element off a 16-byte boundary, inside a
    buffer of a NaN payload: the credit of days reads what the same launch wrote, never the payload; everything outside
    out[k][p][0:n] keeps it bit for bit."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    L_ = _lib.load()
    n = 257
    X = _field(n, dtype, seed=3)
    thr = np.ascontiguousarray(THR9, dtype=np.float64)
    for name in ("4-1-0-5", "1-1-1-1-6", "9-8-0"):
        rb, rows = LISTS[name]
        rbd, rwd = _lists_dev(torch, name)
        P = len(rb) - 1
        for pad in _pads(n, dtype):
            Xd = _strided(torch, X, pad)
            for stat, code, minlen in (("days", _lib.SPELL_DAYS, 6), ("days", _lib.SPELL_DAYS, 3), ("longest", _lib.SPELL_LONGEST, 1)):
                lay = RL.out_layout(9, P, n, 1)
                buf = torch.empty(lay.total, dtype=Xd.dtype, device="cuda")
                bt = torch.int32 if buf.element_size() == 4 else torch.int64
                buf.view(bt).fill_(RL.SENTINEL[buf.element_size()])
                status = torch.zeros(1, dtype=torch.int32, device="cuda")
                fn = getattr(L_, "wagg_spell_span_" + ("f32" if dtype == np.float32 else "f64"))
                vp = C.c_void_p
                _lib.check(fn(vp(Xd.data_ptr()), T, n, Xd.stride(0), vp(rbd.data_ptr()), vp(rwd.data_ptr()), P, len(rows), None, None, 0.0,
                              thr.ctypes.data_as(C.POINTER(C.c_double)), 9, minlen, code, 0, _lib.PERIOD_ROWS_CHECKED,
                              vp(buf.data_ptr() + lay.start * buf.element_size()), lay.ldo, lay.pstride, vp(status.data_ptr()), None, 0,
                              engine._stream_handle(None)), "wagg_spell_span")
                torch.cuda.synchronize()
                bits = buf.view(bt).cpu().numpy()
                idx = RL.inside_index(lay)
                outside = np.ones(lay.total, dtype=bool)
                outside[idx.ravel()] = False
                assert not (outside & (bits != RL.SENTINEL[buf.element_size()])).any(), (name, pad, stat, minlen)
                got = bits[idx].view(dtype).astype(np.float64)
                RL.exact(got, spell_span_ref(X, rb, rows, 0.0, THR9, minlen, stat), (name, pad, stat, minlen))
                assert int(status.item()) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_public_call(torch_cuda, segment_plans, dtype):
    """tas_spell_aggregate(span="record") on a synthetic grid with a segment table, a Kelvin-shifted field and period="month"
    (31 days, then 9): every statistic against the restatement of the per-cell counts aggregated by the fp64 oracle, at the
    project's 1e-4 (fp32) / 1e-6 (fp64); cells="all" and "referenced", device- and host-resident; attrs["span"]; a counted
    +-inf raises; span="period" stays what it was."""
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
    for stat, side, L in (("days", "above", 3), ("events", "above", 2), ("longest", "below", 3), ("days", "below", 6)):
        kw = dict(stat=stat, side=side, min_length=L)
        eff = 1 if stat == "longest" else L
        cells = spell_span_ref(flat, rb, rows, -273.15, thr, eff, stat, side)                  # (n_thr, P, G)
        assert (cells != spell_ref(flat, rb, rows, -273.15, thr, eff, stat, side)).any()      # runs do cross the month's end
        want = np.stack([O.agg_coded(cells[k], c.cell, c.code, c.w_eff, c.R) for k in range(len(thr))])
        out = call(span="record", **kw)
        v = out["tas-spell"]
        assert v.dims == ("threshold", "period", "reg") and v.attrs["span"] == "record" and v.attrs["stat"] == stat
        got = v.values
        assert got.dtype == dtype and got.shape == (len(thr), 2, c.R) and np.isnan(got[:, :, c.R - 1]).all()
        _rel_ok(got, want, c.rtol)
        np.testing.assert_array_equal(got[0], got[2])
        ref = call(cells="referenced", span="record", **kw)["tas-spell"].values
        _rel_ok(ref, want, c.rtol)
        np.testing.assert_array_equal(ref, got)
        np.testing.assert_array_equal(call(ds(device=False), span="record", **kw)["tas-spell"].values, got)
        np.testing.assert_array_equal(call(ds(device=False), cells="referenced", span="record", **kw)["tas-spell"].values, ref)
        old = call(**kw)
        assert old["tas-spell"].attrs["span"] == "period"
        np.testing.assert_array_equal(old["tas-spell"].values, call(span="period", **kw)["tas-spell"].values)
        cut = spell_ref(flat, rb, rows, -273.15, thr, eff, stat, side)
        _rel_ok(old["tas-spell"].values, np.stack([O.agg_coded(cut[k], c.cell, c.code, c.w_eff, c.R) for k in range(len(thr))]), c.rtol)
    hit = c.tas.copy()
    hit.reshape(Tn, c.G)[3, int(c.cell[0])] = np.inf
    for cells_kw in ("all", "referenced"):
        with pytest.raises(ValueError, match="inf"):
            call(ds(f=hit), cells=cells_kw, stat="days", side="below", span="record")


@pytest.mark.parametrize("leap_days", ["keep", "drop"])
def test_cdd_over_new_year(torch_cuda, leap_days):
    """CDD: pr-like values (mm/day) on 20 .. 31 December and 1 .. 12 January, two years of 12 days each, one cell per region.
    A dry run from 27 December to 5 January is one spell of 10 days: the years report 5 and 10, where the truncating call
    reports 5 and 5; CWD of the wet days around it likewise."""
    import pandas as pd
    from climate_toolbox_amd import minixr, tas_spell_aggregate
    torch = torch_cuda
    time = np.datetime64("2001-12-20") + np.arange(24)
    lat, lon = np.array([0.0, 0.5]), np.array([10.0, 10.5])
    pr = np.full((24, 2, 2), 4.0, dtype=np.float32)
    pr[7:17, 0, 0] = 0.2                                     # 27 December .. 5 January: dry
    pr[10:12, 0, 1] = 0.0                                    # 30, 31 December
    pr[12:15, 1, 0] = 0.99                                   # 1 .. 3 January (0.99 mm is dry, 1.0 is wet)
    pr[15, 1, 0] = 1.0
    df = pd.DataFrame({"lat": [0.0, 0.0, 0.5, 0.5], "lon": [10.0, 10.5, 10.0, 10.5], "areawt": 1.0, "popwt": 1.0, "reg": [0, 1, 2, 3]})
    ds = minixr.Dataset({"pr": (("time", "lat", "lon"), torch.from_numpy(pr).cuda())}, coords={"time": time, "lat": lat, "lon": lon})
    kw = dict(tas="pr", stat="longest", period="year", leap_days=leap_days)
    cdd = tas_spell_aggregate(ds, [1.0], "popwt", "reg", df, side="below", span="record", **kw)["tas-spell"].values[0]
    cut = tas_spell_aggregate(ds, [1.0], "popwt", "reg", df, side="below", **kw)["tas-spell"].values[0]
    cwd = tas_spell_aggregate(ds, [1.0], "popwt", "reg", df, side="above", span="record", **kw)["tas-spell"].values[0]
    assert cdd.shape == (2, 4)                               # (period, region): one cell per region, in the table's order
    assert cdd.tolist() == [[5, 2, 0, 0], [10, 0, 3, 0]]
    assert cut.tolist() == [[5, 2, 0, 0], [5, 0, 3, 0]]
    assert cwd.tolist() == [[7, 10, 12, 12], [7, 12, 9, 24]]
