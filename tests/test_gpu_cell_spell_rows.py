"""Spells against per-cell thresholds with a plane PER ROW on the GPU (run with -m gpu): wagg_row_cell_spells_* through
relative.cell_spell_reduce(plane_of_row=) against the NumPy restatement tests/cell_spell_rows_ref.py, its tie to the by-period call,
its layouts, special values and plane checks, the calendar-day baseline identity, and tas_relative_spell_aggregate(planes=
"calendar_day") on a segment table against that restatement aggregated by the fp64 oracle.

Counts are integers and the two sums are sequential fp64 additions: both are compared EXACTLY (bits), never by tolerance; only the
weighted mean of the public call rounds.  The kernel cases share tests/test_gpu_spell.py's shape: T = 23 rows, three periods whose
lists hold 9, 8 and 0 entries with a gap after row 3; n in {5, 257, 1029}: VEC = 1 alone, one block's ragged tail, a second
column block.  The planes change on every row, also inside a run."""
import ctypes as C

import numpy as np
import pytest

from tests import rowlist_layout as RL
from tests.cell_spell_ref import cell_spell_ref
from tests.cell_spell_rows_ref import cell_spell_rows_ref
from tests.spell_ref import WIN_INVERT, WIN_NULL, in_season
from tests.test_gpu_cell_spell import _dev_thr, _same, _tdt, _thr
from tests.test_gpu_packed_totals import _Sparse, segment_plans  # noqa: F401
from tests.test_gpu_spell import OPEN, RB, ROWS, T, _field, _pads, _strided

pytestmark = pytest.mark.gpu

NS = (5, 257, 1029)
SIDES = ("above", "below")
STATS = (("days", 1), ("days", 3), ("events", 3), ("longest", 1), ("amount", 1), ("excess", 1))
PERIOD_OF_ROW = np.repeat([0, 1, 2], [10, 8, 5])                                          # rows 0..9 | 10..17 | 18..22


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _row_planes(M):
    """another plane on every row, every plane used: consecutive rows (a run) never share one for M > 1"""
    return ((np.arange(T) * 5 + 1) % M).astype(np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_results_equal_the_restatement(torch_cuda, dtype, n):
    """All five statistics, both sides, min_length 1 and 3, K in {1, 3, 5, 9} -- a ragged first group, a full group plus a ragged
    one, three groups -- with 4 planes that change on every row; offset 0 and a Kelvin offset (the comparison value formed per
    row, the sums' two roundings); rows and thresholds 16-byte aligned and not."""
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    M = 4
    pmap = _row_planes(M)
    X0 = _field(n, dtype, seed=n)
    for off in (0.0, -273.15):
        X = X0 if off == 0.0 else (X0.astype(np.float64) + 273.15).astype(dtype)
        for pad in _pads(n, dtype):
            Xd = _strided(torch, X, pad)
            for K in (1, 3, 5, 9):
                thr = _thr(n, dtype, K, M, seed=7 * n + K)
                thr_d = _dev_thr(torch, thr, pad_n=pad)
                for side in SIDES:
                    for stat, L in (STATS if K in (1, 5) or off != 0.0 else STATS[1:2] + STATS[5:]):
                        what = (n, off, pad, K, side, stat, L)
                        got, st = cell_spell_reduce(Xd, RB, ROWS, off, thr_d, min_length=L, stat=stat, side=side, plane_of_row=pmap)
                        assert got.shape == (K, 3, n) and got.dtype == _tdt(torch, dtype) and int(st.item()) == 0, what
                        want = cell_spell_rows_ref(X, RB, ROWS, off, thr, pmap, L, stat, side)
                        _same(got, want, dtype, what)
                        assert (got[:, 2] == 0).all(), what                               # the empty list
    # the planes matter: the by-period restatement with any one plane is another result
    assert not np.array_equal(want, cell_spell_ref(X, RB, ROWS, off, thr[:, :1], None, L, stat, side))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_tie_with_the_by_period_call(torch_cuda, dtype, n):
    """plane_of_row[t] = the plane of t's period: bit-equal to cell_spell_reduce(plane_of_period=), with and without a season
    that leaves every cell a counted entry in every non-empty period, with an offset; and all planes identical: bit-equal to the
    one-plane call.  (The empty third period is 0 in both: the thresholds hold no NaN.)"""
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    X = (_field(n, dtype, seed=3 * n).astype(np.float64) + 273.15).astype(dtype)
    K, M, pper = 5, 2, [1, 0, 1]
    thr = _thr(n, dtype, K, M, seed=n)
    prow = np.asarray(pper)[PERIOD_OF_ROW]
    same = np.ascontiguousarray(np.broadcast_to(thr[:, :1], (K, 3, n)))
    doy = np.arange(100, 100 + T)
    win = np.where(np.arange(n) % 3 == 0, OPEN, 101 | 112 << 10).astype(np.int32)      # rows 1..12: counted days in both periods
    for pad in _pads(n, dtype):
        Xd, thr_d, same_d = _strided(torch, X, pad), _dev_thr(torch, thr, pad_n=pad, pad_m=1), _dev_thr(torch, same, pad_n=pad)
        for kw in ({}, dict(doy=doy, windows=win)):
            for off in (0.0, -273.15):
                for side in SIDES:
                    for stat, L in STATS:
                        args = dict(min_length=L, stat=stat, side=side, **kw)
                        what = (n, pad, bool(kw), off, side, stat, L)
                        want, _ = cell_spell_reduce(Xd, RB, ROWS, off, thr_d, pper, **args)
                        got, st = cell_spell_reduce(Xd, RB, ROWS, off, thr_d, plane_of_row=prow, **args)
                        assert torch.equal(got, want) and int(st.item()) == 0, what
                        one, _ = cell_spell_reduce(Xd, RB, ROWS, off, same_d[:, :1], **args)
                        got, _ = cell_spell_reduce(Xd, RB, ROWS, off, same_d, plane_of_row=_row_planes(3), **args)
                        assert torch.equal(got, one), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_layouts(torch_cuda, dtype, n):
    """thr strided in K and M with a padded ldt, the field pitched, the result padded, poison behind every padding
    (tests/rowlist_layout.py's buffers): a read of a pad would make days hot or set status bit 0, a write erases a sentinel.  A
    plane pitch, a level pitch and a threshold base that are no multiple of a piece take the VEC = 1 route: same bits."""
    from climate_toolbox_amd import _lib
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    L = _lib.load()
    X = _field(n, dtype, seed=13 * n)
    K, M = 5, 3
    pmap = _row_planes(M)
    thr = _thr(n, dtype, K, M, seed=n)
    tdt = _tdt(torch, dtype)
    fn = L.wagg_row_cell_spells_f32 if dtype == np.float32 else L.wagg_row_cell_spells_f64
    rb_d = torch.from_numpy(RB.astype(np.int32)).cuda()
    rw_d = torch.from_numpy(ROWS.astype(np.int32)).cuda()
    pm_d = torch.from_numpy(pmap.astype(np.int32)).cuda()
    ptr = lambda t, at=0: C.c_void_p(t.data_ptr() + at * t.element_size())
    v = RL.vec(dtype)
    for stat, Lm, side in (("days", 2, "above"), ("excess", 1, "below")):
        want = cell_spell_rows_ref(X, RB, ROWS, 0.0, thr, pmap, Lm, stat, side)
        plain, _ = cell_spell_reduce(_strided(torch, X, 0), RB, ROWS, 0.0, torch.from_numpy(thr).cuda(), min_length=Lm, stat=stat,
                                     side=side, plane_of_row=pmap)
        _same(plain, want, dtype, (n, stat, "contiguous"))
        for pad in _pads(n, dtype):
            ldx = n + pad + v                                                             # (wide for the first pad, not for the second)
            flat, start = RL.poisoned(X, np.ones(X.shape, dtype=bool), ldx, 0)
            xbuf = torch.from_numpy(flat).cuda()
            assert (RL.GUARD * flat.itemsize) % 16 == 0
            thr_d = _dev_thr(torch, thr, pad_n=pad + v, pad_m=2)
            lay = RL.out_layout(K, 3, n, 0)
            sent = np.array([RL.SENTINEL[flat.itemsize]], dtype=np.uint32 if flat.itemsize == 4 else np.uint64).view(dtype)[0]
            obuf = torch.from_numpy(np.full(lay.total, sent, dtype=dtype)).cuda()
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            rc = fn(ptr(xbuf, start), T, n, ldx, ptr(rb_d), ptr(rw_d), 3, len(ROWS), None, None, 0.0, ptr(thr_d), K, int(thr_d.stride(1)),
                    int(thr_d.stride(0)), ptr(pm_d), M, Lm, {"days": 0, "excess": _lib.CELL_SPELL_EXCESS}[stat], 0 if side == "above" else 1,
                    _lib.PERIOD_ROWS_CHECKED, ptr(obuf, lay.start), lay.ldo, lay.pstride, ptr(status), None, 0, None)
            assert rc == 0, L.wagg_last_error()
            torch.cuda.synchronize()
            o = obuf.cpu().numpy()
            inside = RL.inside_index(lay)
            assert int(status.item()) == 0, (n, pad, stat)
            np.testing.assert_array_equal(o[inside], plain.cpu().numpy(), err_msg=repr((n, pad, stat)))
            rest = np.ones(lay.total, dtype=bool)
            rest[inside.reshape(-1)] = False
            bits = np.uint32 if flat.itemsize == 4 else np.uint64
            assert (o[rest].view(bits) == RL.SENTINEL[flat.itemsize]).all(), (n, pad, stat)
        # field and threshold base 16-byte aligned, but the thresholds' plane pitch (then their level pitch) no multiple of a piece
        Xa = _strided(torch, X, _pads(n, dtype)[0])
        for pad_n, extra in ((_pads(n, dtype)[1], 0), (_pads(n, dtype)[0], 1)):
            buf = torch.full((K * (M * (n + pad_n) + extra),), float("-inf"), dtype=tdt, device="cuda")
            view = buf.as_strided((K, M, n), (M * (n + pad_n) + extra, n + pad_n, 1))
            view.copy_(torch.from_numpy(thr))
            assert view.data_ptr() % 16 == 0 and Xa.stride(0) % v == 0 and (view.stride(1) % v != 0 or view.stride(0) % v != 0)
            got, st = cell_spell_reduce(Xa, RB, ROWS, 0.0, view, min_length=Lm, stat=stat, side=side, plane_of_row=pmap)
            assert torch.equal(got, plain) and int(st.item()) == 0, (n, stat, "pitch", pad_n, extra)
        # the thresholds one element off a 16-byte boundary, the field aligned
        flat1 = torch.full((K * M * n + 1,), float("-inf"), dtype=tdt, device="cuda")
        flat1[1:] = torch.from_numpy(thr).cuda().reshape(-1)
        odd = flat1[1:].view(K, M, n)
        assert odd.data_ptr() % 16 != 0
        got, st = cell_spell_reduce(Xa, RB, ROWS, 0.0, odd, min_length=Lm, stat=stat, side=side, plane_of_row=pmap)
        assert torch.equal(got, plain) and int(st.item()) == 0, (n, stat, "odd base")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(torch_cuda, dtype):
    """A NaN threshold on one day makes that cell, level and period NaN and leaves the others alone; on a day the cell is out of
    season it changes nothing; +-inf thresholds compare as they compare; a NaN day ends a run; an in-season +-inf sets bit 0; a
    row gap resets runs; an empty list gives 0."""
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    n, M = 9, 3
    pmap = (np.arange(T) % M).astype(np.int64)
    X = np.full((T, n), 9.0, dtype=dtype)
    X[2, 1] = np.nan
    thr = np.full((2, M, n), 5.0, dtype=dtype)
    thr[1, :, 5], thr[1, :, 6] = np.inf, -np.inf
    thr[0, 2, 4] = np.nan                                                                 # level 0, plane 2 (rows 2, 5, 8 | 11, 14, 17), cell 4
    thr[1, 1, 7] = np.nan                                                                 # level 1, plane 1: rows 1, 7 | 10, 13, 16 (row 4 is not listed)
    Xd = torch.from_numpy(X).cuda()
    thr_d = torch.from_numpy(thr).cuda()
    for stat in ("days", "events", "longest", "amount", "excess"):
        for side in SIDES:
            got, st = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, stat=stat, side=side, plane_of_row=pmap)
            assert int(st.item()) == 0
            g = got.cpu().numpy()
            assert np.isnan(g[0, :2, 4]).all() and np.isnan(g[1, :2, 7]).all() and np.isnan(g).sum() == 4, (stat, side)
            assert (g[:, 2] == 0).all()                                                   # the empty list: 0, NaN thresholds or not
            _same(got, cell_spell_rows_ref(X, RB, ROWS, 0.0, thr, pmap, 1, stat, side), dtype, (stat, side))
    days, _ = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, plane_of_row=pmap)
    assert days[1, :, 5].tolist() == [0, 0, 0] and days[1, :, 6].tolist() == [9, 8, 0] and days[0, :, 1].tolist() == [8, 8, 0]
    longest, _ = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, stat="longest", plane_of_row=pmap)
    assert longest[0, :, 0].tolist() == [5, 8, 0] and longest[0, :, 1].tolist() == [5, 8, 0]      # rows 0-3 | 5-9: the gap; the NaN day at row 2
    # a NaN threshold only on days the cell is out of season changes nothing; on a counted day it is NaN for that period only
    doy = np.arange(100, 100 + T)
    win = np.full(n, 100 | 110 << 10, dtype=np.int32)                                     # rows 0..10 in season
    late = np.full((2, M, n), 5.0, dtype=dtype)
    only = np.full(T, 0, dtype=np.int64)
    only[[12, 13]] = 1                                                                    # plane 1 on rows 12, 13 alone: out of season
    late[0, 1, 3] = np.nan
    kw = dict(doy=doy, windows=win)
    clean, _ = cell_spell_reduce(Xd, RB, ROWS, 0.0, torch.full((2, M, n), 5.0, dtype=Xd.dtype, device="cuda"), plane_of_row=only, **kw)
    got, st = cell_spell_reduce(Xd, RB, ROWS, 0.0, torch.from_numpy(late).cuda(), plane_of_row=only, **kw)
    assert torch.equal(got, clean) and int(st.item()) == 0 and not torch.isnan(got).any()
    only[[12, 13]], only[10] = 0, 1                                                       # ... on row 10, the second period's one counted day
    got, _ = cell_spell_reduce(Xd, RB, ROWS, 0.0, torch.from_numpy(late).cuda(), plane_of_row=only, **kw)
    g = got.cpu().numpy()
    assert np.isnan(g[0, 1, 3]) and np.isnan(g).sum() == 1
    _same(got, cell_spell_rows_ref(X, RB, ROWS, 0.0, late, only, 1, "days", "above", doy, win), dtype, "counted NaN")
    for v in (np.inf, -np.inf):
        for t, counted in ((6, True), (14, False)):
            Xi = X.copy()
            Xi[t, 3] = v
            for skw in (kw, {}):
                got, st = cell_spell_reduce(torch.from_numpy(Xi).cuda(), RB, ROWS, 0.0, thr_d, min_length=2, plane_of_row=pmap, **skw)
                assert int(st.item()) == (1 if counted or not skw else 0), (v, t, bool(skw))
                want = cell_spell_rows_ref(Xi, RB, ROWS, 0.0, thr, pmap, 2, "days", "above", skw.get("doy"), skw.get("windows"))
                _same(got, want, dtype, (v, t))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plane_checks(torch_cuda, dtype):
    """An out-of-range plane on a listed row raises for host arrays, and for device arrays with checked=False; with checked=True
    it gives NaN for that period only, and status bit 2; on an unlisted row (row 4, rows 18..22) it is accepted."""
    from climate_toolbox_amd import _lib, engine
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    n, M, K = 261, 2, 5
    X = _field(n, dtype, seed=4)
    thr = _thr(n, dtype, K, M, seed=9)
    Xd, thr_d = torch.from_numpy(X).cuda(), torch.from_numpy(thr).cuda()
    rb_d, rw_d = engine.period_lists(RB, ROWS, T)
    good = (np.arange(T) % M).astype(np.int64)
    unlisted = good.copy()
    unlisted[[4, 18, 20, 22]] = [M, -1, 99, -7]
    want = cell_spell_rows_ref(X, RB, ROWS, 0.0, thr, good, 2)
    for pm in (unlisted, torch.from_numpy(unlisted.astype(np.int32)).cuda()):
        for lists, chk in (((RB, ROWS), False), ((rb_d, rw_d), False), ((rb_d, rw_d), True)):
            got, st = cell_spell_reduce(Xd, *lists, 0.0, thr_d, min_length=2, checked=chk, plane_of_row=pm)
            assert int(st.item()) == 0
            _same(got, want, dtype, "unlisted")
    for row, val, p_bad in ((12, M, 1), (3, -1, 0)):
        bad = good.copy()
        bad[row] = val
        bad_d = torch.from_numpy(bad.astype(np.int32)).cuda()
        with pytest.raises(ValueError, match="plane_of_row"):
            cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, plane_of_row=bad)
        with pytest.raises(_lib.WaggError, match="plane_of_row"):
            cell_spell_reduce(Xd, rb_d, rw_d, 0.0, thr_d, plane_of_row=bad_d)
        for stat in ("days", "excess"):
            got, st = cell_spell_reduce(Xd, rb_d, rw_d, 0.0, thr_d, stat=stat, checked=True, plane_of_row=bad_d)
            g = got.cpu().numpy()
            assert int(st.item()) == 4 and np.isnan(g[:, p_bad]).all() and np.isnan(g).sum() == K * n, (row, stat)
            _same(got, cell_spell_rows_ref(X, RB, ROWS, 0.0, thr, bad, 1, stat), dtype, (row, stat))
    with pytest.raises(ValueError, match="exclude"):
        cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, [0, 1, 0], plane_of_row=good)
    with pytest.raises(ValueError, match="23 entries"):
        cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, plane_of_row=good[:-1])
    with pytest.raises(TypeError, match="plane_of_row"):
        cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, plane_of_row=good.astype(np.float64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_seasons(torch_cuda, dtype, n):
    """tests/test_gpu_cell_spell.py's season case with a plane per row: open, null, ordinary and inverted windows, a day in no
    season, and cells 4..7 out of season together on row 6 -- the piece is read neither from the field nor from the thresholds and
    the runs end all the same.  Poison out of season, in the field and in the thresholds, changes nothing."""
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    M = 3
    pmap = _row_planes(M)
    X = _field(n, dtype, seed=11 * n)
    X[:, 4:8] = 9.0
    doy = np.arange(100, 100 + T)
    doy[12] = 2000
    kinds = np.array([OPEN, 1 | 0 << 10 | WIN_NULL, 102 | 107 << 10, 103 | 105 << 10 | WIN_INVERT, 300 | 320 << 10], dtype=np.int32)
    win = kinds[np.arange(n) % 5]
    win[4:8] = 106 | 106 << 10 | WIN_INVERT
    thr = _thr(n, dtype, 2, M, seed=n)
    thr[:, :, 4:8] = 5.0
    season = np.stack([in_season(int(doy[t]), win) for t in range(T)])
    poison = np.array([np.nan, np.inf, -np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 4]
    Xp = np.where(season, X, poison).astype(dtype)
    thr_p = thr.copy()                                                                    # NaN thresholds wherever a cell is never counted
    for m in range(M):
        never = ~season[[t for t in ROWS if pmap[t] == m]].any(0)
        thr_p[:, m, never] = np.nan
    assert np.isnan(thr_p).any()
    for pad in _pads(n, dtype):
        Xd, Xpd = _strided(torch, X, pad), _strided(torch, Xp, pad)
        thr_d, thr_pd = _dev_thr(torch, thr, pad_n=pad), _dev_thr(torch, thr_p, pad_n=pad)
        for side in SIDES:
            for stat, L in (("days", 1), ("days", 3), ("events", 2), ("longest", 1), ("amount", 1), ("excess", 1)):
                kw = dict(min_length=L, stat=stat, side=side, doy=doy, windows=win, plane_of_row=pmap)
                got, st = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, **kw)
                assert int(st.item()) == 0
                _same(got, cell_spell_rows_ref(X, RB, ROWS, 0.0, thr, pmap, L, stat, side, doy, win), dtype, (n, pad, side, stat, L))
                g2, st = cell_spell_reduce(Xpd, RB, ROWS, 0.0, thr_pd, **kw)
                assert torch.equal(g2, got) and int(st.item()) == 0
    longest = cell_spell_rows_ref(X, RB, ROWS, 0.0, thr, pmap, 1, "longest", "above", doy, win)[0]
    if n > 5:
        assert longest[:, 4].tolist() == [4, 5, 0]                                        # rows 0-3, 5, 7-9 | 10 11, 13-17


def _year_field(rng, T_, n):
    """distinct values per cell (an order with a seasonal cycle), Kelvin"""
    base = 283.0 + 10.0 * np.sin(2 * np.pi * np.arange(T_) / 365.0)[:, None]
    return base + np.argsort(rng.uniform(size=(T_, n)), axis=0) * 0.013 + rng.uniform(0, 0.01, (1, n))


@pytest.mark.parametrize("n", NS)
def test_fp32_kelvin_identity_and_a_pooled_baseline(torch_cuda, n):
    """The baseline of calendar_day_rows(window=1) over one year of the same fp32 Kelvin field is the field: thr == x, so "above"
    counts every valid day and "below" none, exactly, on raw elements with offset 0.  Then a 3-year record with window=5 and q =
    0.5 through engine.quantile_select against the restatement."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.relative import calendar_day_rows, cell_spell_reduce, resolve_row_planes
    torch = torch_cuda
    rng = np.random.default_rng(n)
    time = np.datetime64("2001-01-01") + np.arange(365)
    X = _year_field(rng, 365, n).astype(np.float32)
    X[40, 1] = X[41, 1] = np.nan
    labels, rb, rows = calendar_day_rows(time, window=1)
    Xd = torch.from_numpy(X).cuda()
    thr, st = engine.quantile_select(Xd, rb, rows, 0.0, [0.9], method="linear")
    assert int(st.item()) == 0 and np.array_equal(thr.cpu().numpy()[0], X, equal_nan=True)
    pmap = resolve_row_planes(labels, time)
    assert pmap.tolist() == list(range(365))
    valid = (~np.isnan(X)).sum(0).astype(np.float32)
    year = (np.array([0, 365]), np.arange(365))
    up, _ = cell_spell_reduce(Xd, *year, 0.0, thr, plane_of_row=pmap)
    down, _ = cell_spell_reduce(Xd, *year, 0.0, thr, side="below", plane_of_row=pmap)
    ok = np.ones(n, dtype=bool)
    ok[1] = False                                                                         # (cell 1: a NaN threshold on a counted day)
    up, down = up.cpu().numpy()[0, 0], down.cpu().numpy()[0, 0]
    assert np.array_equal(up[ok], valid[ok]) and (valid[ok] == 365).all() and np.isnan(up[1]) and np.isnan(down[1])
    assert (down[ok] == 0).all()
    # three years, pooled over 5 days, the median: against the restatement, with the WSDI run length
    T3 = 3 * 365 + 1
    time3 = np.datetime64("2003-01-01") + np.arange(T3)                                   # (2004 holds a 29 February)
    X3 = _year_field(rng, T3, n).astype(np.float32)
    labels, rb, rows = calendar_day_rows(time3, window=5)
    assert len(labels) == 366
    X3d = torch.from_numpy(X3).cuda()
    thr3, st = engine.quantile_select(X3d, rb, rows, 0.0, [0.5], method="linear")
    pmap = resolve_row_planes(labels, time3)
    from climate_toolbox_amd.periods import period_rows
    _, yrb, yrows = period_rows(time3, "year")
    for stat, L in (("days", 1), ("days", 6), ("excess", 1)):
        got, st = cell_spell_reduce(X3d, yrb, yrows, 0.0, thr3, min_length=L, stat=stat, plane_of_row=pmap)
        assert int(st.item()) == 0
        want = cell_spell_rows_ref(X3, yrb, yrows, 0.0, thr3.cpu().numpy(), pmap, L, stat)
        _same(got, want, np.float32, (n, stat, L))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_public_call(torch_cuda, segment_plans, dtype):
    """tas_relative_spell_aggregate(planes="calendar_day") on a small grid with a segment table: two years, 2004 with its 29
    February, a Kelvin-shifted field and a calendar-day baseline of the same variable (offset exactly 0), for both leap_days
    values: against the restatement aggregated by the fp64 oracle at the project's 1e-4 (fp32) / 1e-6 (fp64); cells="all" and
    "referenced"; a season; a listed day without a plane is ValueError naming the date."""
    from climate_toolbox_amd.relative import cell_quantiles, resolve_row_planes
    from climate_toolbox_amd.periods import period_rows
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_relative_spell_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=31)
    Tn = 366 + 365
    rng = np.random.default_rng(8)
    c.T, c.time = Tn, np.datetime64("2004-01-01") + np.arange(Tn)
    tas = _year_field(rng, Tn, c.G).astype(dtype)
    tas[70, c.cell[3]] = np.nan
    c.tas = tas.reshape(Tn, c.nlat, c.nlon)
    ds = lambda: convert_kelvin_to_celsius(c.dataset(torch), "tas")
    agg = lambda cells: np.stack([O.agg_coded(cells[k], c.cell, c.code, c.w_eff, c.R) for k in range(cells.shape[0])])

    def ok(got, want, cells):
        bound = agg(np.abs(np.nan_to_num(cells, nan=0.0)))
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        fin = ~np.isnan(want)
        assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= c.rtol * bound[fin] + 1e-300).all()
    for leap in ("keep", "drop"):
        base = cell_quantiles(ds(), [0.5, 0.9], period="calendar_day", window=5, leap_days=leap)
        assert base.M == (366 if leap == "keep" else 365) and base.shift == -273.15 and base.labels[0] == 101 and base.labels[-1] == 1231
        assert (229 in base.labels.tolist()) == (leap == "keep")
        keep = np.ones(Tn, dtype=bool) if leap == "keep" else ~((c.time.astype("datetime64[M]").astype(int) % 12 == 1)
                                                                 & ((c.time - c.time.astype("datetime64[M]")).astype(int) == 28))
        flat, time = tas[keep], c.time[keep]
        _, rb, rows = period_rows(time, "year")
        raw = base.values.cpu().numpy().reshape(2, base.M, c.G)
        pmap = resolve_row_planes(base.labels, time)
        from climate_toolbox_amd import seasons
        sw = seasons.SeasonWindows(np.full((c.nlat, c.nlon), 100 | 250 << 10, dtype=np.int32), c.lat, c.lon)
        for stat, side, L, kw in (("days", "above", 1, {}), ("days", "above", 6, {}), ("excess", "below", 1, {}),
                                  ("events", "above", 2, dict(season=sw))):
            doy = win = None
            if kw:
                doy = seasons.day_of_year(time)
                win = np.full(c.G, 100 | 250 << 10, dtype=np.int32)
            cells = cell_spell_rows_ref(flat, rb, rows, 0.0, raw, pmap, L, stat, side, doy, win)
            assert len(np.unique(cells[~np.isnan(cells)])) > 2
            want = agg(cells)
            call = lambda **more: tas_relative_spell_aggregate(ds(), base, "popwt", "reg", c.df, period="year", planes="calendar_day",
                                                               stat=stat, side=side, min_length=L, leap_days=leap, **kw, **more)
            out = call()
            v = out["tas-relative-spell"]
            assert v.dims == ("threshold", "period", "reg") and list(out["period"].values) == [2004, 2005]
            assert list(out["threshold"].values) == [0.5, 0.9] and v.values.shape == (2, 2, c.R)
            ok(v.values, want, cells)
            ok(call(cells="referenced")["tas-relative-spell"].values, want, cells)
    # the data keep their 29 February, the baseline was built without it
    with pytest.raises(ValueError, match="2004-02-29"):
        tas_relative_spell_aggregate(ds(), base, "popwt", "reg", c.df, period="year", planes="calendar_day", min_length=1)
    with pytest.raises(ValueError, match="window"):
        cell_quantiles(ds(), [0.9], period="month", window=5)
