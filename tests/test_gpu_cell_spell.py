"""Spells against per-cell thresholds on the GPU (run with -m gpu): wagg_cell_spells_* through relative.cell_spell_reduce against
the NumPy restatement tests/cell_spell_ref.py, its laws against engine.spell_reduce and engine.quantile_select, and
tas_relative_spell_aggregate on a segment table against that restatement aggregated by the fp64 oracle.

Counts are integers and the two sums are sequential fp64 additions: both are compared EXACTLY (bits), never by tolerance; only
the weighted mean of the public call rounds.  The kernel cases share tests/test_gpu_spell.py's shape: T = 23 rows, three periods
whose lists hold 9, 8 and 0 entries with a gap after row 3, n in {1, 3, 4, 5, 257, 1029}."""
import ctypes as C

import numpy as np
import pytest

from tests.cell_spell_ref import cell_spell_ref
from tests.spell_ref import WIN_INVERT, WIN_NULL, in_season
from tests.test_gpu_packed_totals import _Sparse, segment_plans  # noqa: F401
from tests.test_gpu_parity import _rel_ok
from tests.test_gpu_spell import NS, OPEN, RB, ROWS, T, _field, _pads, _strided

pytestmark = pytest.mark.gpu

SIDES = ("above", "below")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _tdt(torch, dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


def _thr(n, dtype, K, M, seed):
    """thresholds inside the field's range 0..10, another number in every cell, plane and level"""
    return np.random.default_rng(seed).uniform(1.0, 9.5, (K, M, n)).astype(dtype)


def _dev_thr(torch, host, pad_n=0, pad_m=0, fill=-np.inf):
    """(K, M, n) on the device inside a (K, M + pad_m, n + pad_n) buffer of ``fill``: strided in both leading dims"""
    K, M, n = host.shape
    buf = torch.full((K, M + pad_m, n + pad_n), fill, dtype=_tdt(torch, host.dtype), device="cuda")
    buf[:, :M, :n] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return buf[:, :M, :n]


def _same(got, want, dtype, what):
    """bit equality with the restatement cast to the element type as the kernel casts on its store (NaN equals NaN)"""
    got = got.cpu().numpy()
    with np.errstate(over="ignore"):
        want = want.astype(dtype)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, "%r: %d values differ, first at (level, period, cell) %r: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


CASES = ((1, 1, None), ("G", 2, [1, 0, 1]), ("G+1", 3, None), (64, 2, [0, 1, 0]))      # (K, M, plane of every period)
STATS = (("days", 1), ("days", 2), ("events", 2), ("longest", 1), ("amount", 1), ("excess", 1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_results_equal_the_restatement(torch_cuda, dtype, n):
    """Every statistic, both sides, K in {1, group, group + 1, 64}, one plane, two planes with a map that uses both, and a
    plane per period with a NULL map; rows and thresholds 16-byte aligned and not."""
    from climate_toolbox_amd import _lib
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    X = _field(n, dtype, seed=n)
    G = _lib.CELL_SPELL_GROUP
    for pad in _pads(n, dtype):
        Xd = _strided(torch, X, pad)
        for K, M, pmap in CASES:
            K = {"G": G, "G+1": G + 1}.get(K, K)
            thr = _thr(n, dtype, K, M, seed=7 * n + K)
            thr_d = _dev_thr(torch, thr, pad_n=pad)
            for side in SIDES:
                for stat, L in STATS:
                    what = (n, pad, K, M, side, stat, L)
                    got, st = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, pmap, min_length=L, stat=stat, side=side)
                    assert got.shape == (K, 3, n) and got.dtype == _tdt(torch, dtype) and int(st.item()) == 0, what
                    _same(got, cell_spell_ref(X, RB, ROWS, 0.0, thr, pmap, L, stat, side), dtype, what)
                    assert (got[:, 2] == 0).all(), what                                   # the empty period


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [5, 1029])
def test_sums_with_an_offset_equal_the_restatement_in_their_bits(torch_cuda, dtype, n):
    """amount and excess on a Kelvin field with offset = -273.15 and thresholds in degrees C: the first rounding, (double)x +
    offset, is no identity here, the second, the difference with (double)thr, follows it, and the terms add up in list order --
    the bits of the NumPy loop, on both sides, with and without a season.  (A kernel that formed (x - thr) + offset, fused the two
    operations or left the offset out of the sums would differ in the last bits of the fp64 sums.)"""
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    off = -273.15
    rng = np.random.default_rng(41 * n)
    X = (273.15 + rng.uniform(0.0, 10.0, (T, n))).astype(dtype)
    X[5, 0] = np.nan
    thr = rng.uniform(1.0, 9.5, (5, 2, n)).astype(dtype)
    pmap = [1, 0, 1]
    doy = np.arange(100, 100 + T)
    win = np.where(np.arange(n) % 3 == 0, OPEN, 101 | 112 << 10).astype(np.int32)
    differs = 0
    for pad in _pads(n, dtype):
        Xd, thr_d = _strided(torch, X, pad), _dev_thr(torch, thr, pad_n=pad, pad_m=1)
        for kw in ({}, dict(doy=doy, windows=win)):
            for side in SIDES:
                for stat in ("amount", "excess"):
                    got, st = cell_spell_reduce(Xd, RB, ROWS, off, thr_d, pmap, stat=stat, side=side, **kw)
                    assert int(st.item()) == 0
                    want = cell_spell_ref(X, RB, ROWS, off, thr, pmap, 1, stat, side, kw.get("doy"), kw.get("windows"))
                    _same(got, want, dtype, (n, pad, bool(kw), side, stat))
                    if dtype == np.float64 and stat == "excess" and not kw and side == "above":
                        # the other order of the two operations is another number somewhere: the check above can tell them apart
                        hot = X.astype(np.float64)[ROWS[:9], None, :] >= thr[None, :, 1, :].astype(np.float64) - off
                        a = (X.astype(np.float64)[ROWS[:9], None, :] + off) - thr[None, :, 1, :]
                        b = (X.astype(np.float64)[ROWS[:9], None, :] - thr[None, :, 1, :]) + off
                        differs += int((hot & (a != b)).sum())
    assert dtype != np.float64 or differs > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [5, 257, 1029])
def test_constant_field_is_the_scalar_call_bit_for_bit(torch_cuda, dtype, n):
    """A threshold field that is the same number in every cell gives engine.spell_reduce's planes, with and without a season and
    with a Kelvin offset."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    X = (_field(n, dtype, seed=3 * n) + dtype(273.15)).astype(dtype)
    thr = np.array([5.0, 2.0, 8.75, 5.0, -3.0], dtype=dtype)
    doy = np.arange(100, 100 + T)
    win = np.where(np.arange(n) % 4 == 1, 103 | 109 << 10, OPEN).astype(np.int32)
    field = np.ascontiguousarray(np.broadcast_to(thr[:, None, None], (len(thr), 1, n)))
    for pad in _pads(n, dtype):
        Xd, thr_d = _strided(torch, X, pad), _dev_thr(torch, field, pad_n=pad)
        for kw in ({}, dict(doy=doy, windows=win)):
            for side in SIDES:
                for stat, L in (("days", 1), ("days", 3), ("events", 2), ("longest", 1)):
                    want, _ = engine.spell_reduce(Xd, RB, ROWS, -273.15, thr.astype(np.float64), min_length=L, stat=stat, side=side, **kw)
                    got, st = cell_spell_reduce(Xd, RB, ROWS, -273.15, thr_d, min_length=L, stat=stat, side=side, **kw)
                    assert torch.equal(got, want) and int(st.item()) == 0, (n, pad, bool(kw), side, stat, L)


def test_fp32_kelvin_field_is_classified_as_in_fp64(torch_cuda):
    """tests/test_gpu_spell.py's case of the same name: 35 C on a Kelvin field, values one ulp below, on and one ulp above
    float32(308.15), and per-cell thresholds that straddle 35 by one ulp.  The device's ceilT((double)thr - offset) classifies
    as fp64 would, on both sides, and a constant 35 gives the scalar kernel's bits."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    off = -273.15
    f = np.float32(35.0 - off)
    vals = np.array([np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(1e9))], dtype=np.float32)
    t35 = np.float32(35.0)
    thrs = np.array([np.nextafter(t35, np.float32(0)), t35, np.nextafter(t35, np.float32(100))], dtype=np.float32)
    n = 27 * 5
    X = np.empty((T, n), dtype=np.float32)
    for j in range(n):
        X[:, j] = vals[[(j // 3 ** (t % 3)) % 3 for t in range(T)]]
    X[:, 27:54] = np.roll(X[:, 27:54], 1, axis=0)
    thr = thrs[(np.arange(n) // 9) % 3][None, None, :].copy()                            # every threshold meets every triple of values
    const = np.full((1, 1, n), t35, dtype=np.float32)
    for pad in _pads(n, np.float32):
        Xd = _strided(torch, X, pad)
        for side in SIDES:
            for stat, L in (("days", 1), ("days", 2), ("events", 2), ("longest", 1)):
                got, st = cell_spell_reduce(Xd, RB, ROWS, off, _dev_thr(torch, thr, pad_n=pad), min_length=L, stat=stat, side=side)
                assert int(st.item()) == 0
                _same(got, cell_spell_ref(X, RB, ROWS, off, thr, None, L, stat, side), np.float32, (pad, side, stat, L))
                one, _ = cell_spell_reduce(Xd, RB, ROWS, off, _dev_thr(torch, const, pad_n=pad), min_length=L, stat=stat, side=side)
                assert torch.equal(one, engine.spell_reduce(Xd, RB, ROWS, off, [35.0], min_length=L, stat=stat, side=side)[0])
    # the restatement's rule is the fp64 classification of the exact values
    hot = X[0].astype(np.float64) >= thr[0, 0].astype(np.float64) - off
    assert hot.any() and not hot.all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plane_k_is_the_one_level_call(torch_cuda, dtype):
    """A K-level call equals K one-level calls bit for bit (a ragged last group), counts and sums, under a season."""
    from climate_toolbox_amd import _lib
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    n, K = 257, 2 * _lib.CELL_SPELL_GROUP + 1
    X = _field(n, dtype, seed=7)
    thr = _thr(n, dtype, K, 2, seed=5)
    thr[3] = thr[6]                                                                       # a duplicate level
    doy = np.arange(100, 100 + T)
    win = np.where(np.arange(n) % 3 == 0, OPEN, 101 | 112 << 10).astype(np.int32)
    pmap = [0, 1, 1]
    for pad in _pads(n, dtype):
        Xd, thr_d = _strided(torch, X, pad), _dev_thr(torch, thr, pad_n=pad, pad_m=1)
        for stat, L, side in (("days", 2, "above"), ("events", 2, "below"), ("excess", 1, "above"), ("amount", 1, "below")):
            kw = dict(min_length=L, stat=stat, side=side, doy=doy, windows=win)
            got, _ = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, pmap, **kw)
            for k in range(K):
                one, _ = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d[k:k + 1], pmap, **kw)
                assert torch.equal(got[k], one[0]), (pad, stat, k)
            assert torch.equal(got[3], got[6])
            _same(got, cell_spell_ref(X, RB, ROWS, 0.0, thr, pmap, L, stat, side, doy, win), dtype, (pad, stat))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("season", [False, True])
def test_rank_identity_with_the_period_quantiles(torch_cuda, dtype, season):
    """Distinct values per cell, offset 0, thr = quantile_select(method="higher", q) of the same lists: the days at or above the
    cell's own q-quantile number m - ceil((m - 1) q) exactly, m being the cell's valid days -- and NaN where m = 0."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    n = 1029
    rng = np.random.default_rng(17)
    X = (280.0 + np.argsort(rng.uniform(size=(T, n)), axis=0) * 0.37 + rng.uniform(0, 0.1, (1, n))).astype(dtype)
    assert all(len(np.unique(X[:, j])) == T for j in range(0, n, 97))
    q = [0.9, 0.95, 0.99, 0.0, 1.0, 0.5, 1.0 / 3.0]
    doy = np.arange(100, 100 + T)
    kinds = np.array([OPEN, 1 | 0 << 10 | WIN_NULL, 102 | 107 << 10, 103 | 105 << 10 | WIN_INVERT, 300 | 320 << 10], dtype=np.int32)
    win = kinds[np.arange(n) % 5]
    kw = dict(doy=doy, windows=win) if season else {}
    m = np.zeros((3, n))
    for p in range(3):
        for t in ROWS[RB[p]:RB[p + 1]]:
            m[p] += in_season(int(doy[t]), win) if season else 1
    want = np.stack([np.where(m > 0, m - np.ceil((m - 1) * qk), np.nan) for qk in q])
    assert (m == 0).any() and (want[0][m > 0] >= 1).all()
    for pad in _pads(n, dtype):
        Xd = _strided(torch, X, pad)
        thr, st = engine.quantile_select(Xd, RB, ROWS, 0.0, q, method="higher", **kw)
        assert int(st.item()) == 0
        got, st = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr, min_length=1, stat="days", side="above", **kw)
        assert int(st.item()) == 0
        _same(got, want, dtype, (pad, season))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [5, 257, 1029])
def test_layouts(torch_cuda, dtype, n):
    """thr strided in both leading dims, the field and the result pitched, poison in every pad: -inf in the thresholds' pads (a
    read would make every day hot), +inf in the field's (a read would set status bit 0), a sentinel in the result's (a write would
    erase it).  A threshold base that is not 16-byte aligned beside an aligned field takes the element-wise route: same bits."""
    from climate_toolbox_amd import _lib
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    L = _lib.load()
    X = _field(n, dtype, seed=13 * n)
    K, M, pmap = 5, 2, [1, 0, 1]
    thr = _thr(n, dtype, K, M, seed=n)
    tdt = _tdt(torch, dtype)
    fn = L.wagg_cell_spells_f32 if dtype == np.float32 else L.wagg_cell_spells_f64
    rb_d = torch.from_numpy(RB.astype(np.int32)).cuda()
    rw_d = torch.from_numpy(ROWS.astype(np.int32)).cuda()
    pm_d = torch.from_numpy(np.array(pmap, dtype=np.int32)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for stat, Lm, side in (("days", 2, "above"), ("excess", 1, "below")):
        want = cell_spell_ref(X, RB, ROWS, 0.0, thr, pmap, Lm, stat, side)
        plain, _ = cell_spell_reduce(_strided(torch, X, 0), RB, ROWS, 0.0, torch.from_numpy(thr).cuda(), pmap, min_length=Lm, stat=stat, side=side)
        _same(plain, want, dtype, (n, stat, "contiguous"))
        for pad in _pads(n, dtype):
            xbuf = torch.full((T, n + pad + 4), float("inf"), dtype=tdt, device="cuda")
            xbuf[:, :n] = torch.from_numpy(X).cuda()
            thr_d = _dev_thr(torch, thr, pad_n=pad + 4, pad_m=2)
            ldo, pstride = n + pad + 4, 3 * (n + pad + 4) + 8
            obuf = torch.full((K * pstride,), -12345.0, dtype=tdt, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            rc = fn(ptr(xbuf), T, n, n + pad + 4, ptr(rb_d), ptr(rw_d), 3, len(ROWS), None, None, 0.0, ptr(thr_d), K, int(thr_d.stride(1)),
                    int(thr_d.stride(0)), ptr(pm_d), M, Lm, {"days": 0, "excess": _lib.CELL_SPELL_EXCESS}[stat], 0 if side == "above" else 1,
                    _lib.PERIOD_ROWS_CHECKED, ptr(obuf), ldo, pstride, ptr(status), None, 0, None)
            assert rc == 0, L.wagg_last_error()
            torch.cuda.synchronize()
            o = obuf.cpu().numpy()
            res = np.stack([o[k * pstride:k * pstride + 3 * ldo].reshape(3, ldo) for k in range(K)])
            assert int(status.item()) == 0, (n, pad, stat)
            np.testing.assert_array_equal(res[:, :, :n], plain.cpu().numpy(), err_msg=repr((n, pad, stat)))
            assert (res[:, :, n:] == -12345.0).all() and all((o[k * pstride + 3 * ldo:(k + 1) * pstride] == -12345.0).all() for k in range(K))
        # field and threshold base 16-byte aligned, but the thresholds' plane pitch (then their level pitch) no multiple of a piece
        Xa = _strided(torch, X, _pads(n, dtype)[0])
        v = 16 // np.dtype(dtype).itemsize
        for pad_n, extra in ((_pads(n, dtype)[1], 0), (_pads(n, dtype)[0], 1)):
            buf = torch.full((K * (M * (n + pad_n) + extra),), float("-inf"), dtype=tdt, device="cuda")
            view = buf.as_strided((K, M, n), (M * (n + pad_n) + extra, n + pad_n, 1))
            view.copy_(torch.from_numpy(thr))
            assert view.data_ptr() % 16 == 0 and Xa.stride(0) % v == 0 and (view.stride(1) % v != 0 or view.stride(0) % v != 0)
            got, st = cell_spell_reduce(Xa, RB, ROWS, 0.0, view, pmap, min_length=Lm, stat=stat, side=side)
            assert torch.equal(got, plain) and int(st.item()) == 0, (n, stat, "pitch", pad_n, extra)
        # the thresholds one element off a 16-byte boundary, the field aligned
        flat = torch.full((K * M * n + 1,), float("-inf"), dtype=tdt, device="cuda")
        flat[1:] = torch.from_numpy(thr).cuda().reshape(-1)
        odd = flat[1:].view(K, M, n)
        assert odd.data_ptr() % 16 != 0
        got, st = cell_spell_reduce(_strided(torch, X, _pads(n, dtype)[0]), RB, ROWS, 0.0, odd, pmap, min_length=Lm, stat=stat, side=side)
        assert torch.equal(got, plain) and int(st.item()) == 0, (n, stat, "odd base")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(torch_cuda, dtype):
    """A NaN threshold makes that cell NaN and no other; +-inf thresholds compare as they compare; NaN days are cold; an in-season
    +-inf sets bit 0; a plane index out of range is NaN for the period and bit 2 with checked=True, an error without."""
    from climate_toolbox_amd import _lib, engine
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    n = 9
    X = np.full((T, n), 9.0, dtype=dtype)
    X[2, 1] = np.nan
    thr = np.full((2, 1, n), 5.0, dtype=dtype)
    thr[0, 0, 4], thr[1, 0, 5], thr[1, 0, 6] = np.nan, np.inf, -np.inf
    thr_d = torch.from_numpy(thr).cuda()
    for stat in ("days", "events", "longest", "amount", "excess"):
        for side in SIDES:
            got, st = cell_spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, thr_d, stat=stat, side=side)
            assert int(st.item()) == 0
            g = got.cpu().numpy()
            assert np.isnan(g[0, :, 4]).all() and np.isnan(g).sum() == 3, (stat, side)
            _same(got, cell_spell_ref(X, RB, ROWS, 0.0, thr, None, 1, stat, side), dtype, (stat, side))
    days, _ = cell_spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, thr_d)
    assert days[1, :, 5].tolist() == [0, 0, 0] and days[1, :, 6].tolist() == [9, 8, 0] and days[0, :, 1].tolist() == [8, 8, 0]
    doy = np.arange(100, 100 + T)
    win = np.full(n, 100 | 110 << 10, dtype=np.int32)                                     # rows 0..10 in season
    for v in (np.inf, -np.inf):
        for t, counted in ((6, True), (14, False)):
            Xi = X.copy()
            Xi[t, 3] = v
            for kw in (dict(doy=doy, windows=win), {}):
                got, st = cell_spell_reduce(torch.from_numpy(Xi).cuda(), RB, ROWS, 0.0, thr_d, min_length=2, **kw)
                assert int(st.item()) == (1 if counted or not kw else 0), (v, t, bool(kw))
                _same(got, cell_spell_ref(Xi, RB, ROWS, 0.0, thr, None, 2, "days", "above", kw.get("doy"), kw.get("windows")), dtype, (v, t))
    # plane indices out of range: device lists and a device map
    rb_d, rw_d = engine.period_lists(RB, ROWS, T)
    two = torch.from_numpy(np.concatenate([thr, thr + dtype(1)], axis=1)).cuda()
    for bad in ([0, 2, 1], [0, 1, -1]):
        pm = torch.from_numpy(np.array(bad, dtype=np.int32)).cuda()
        got, st = cell_spell_reduce(torch.from_numpy(X).cuda(), rb_d, rw_d, 0.0, two, pm, checked=True)
        g = got.cpu().numpy()
        p_bad = 1 if bad[1] == 2 else 2
        assert int(st.item()) == 4 and np.isnan(g[:, p_bad]).all() and np.isnan(g).sum() == 2 * n + 2, bad     # (+ the NaN threshold's cell)
        _same(got, cell_spell_ref(X, RB, ROWS, 0.0, np.concatenate([thr, thr + dtype(1)], axis=1), bad), dtype, bad)
        with pytest.raises(_lib.WaggError, match="plane_of_period"):
            cell_spell_reduce(torch.from_numpy(X).cuda(), rb_d, rw_d, 0.0, two, pm)
    with pytest.raises(ValueError, match="plane_of_period"):
        cell_spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, two, [0, 2, 1])
    with pytest.raises(ValueError, match="plane_of_period=None"):
        cell_spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, two)
    with pytest.raises(ValueError, match="amount"):
        cell_spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, thr_d, stat="amount", min_length=2)
    with pytest.raises(TypeError, match="dtype"):
        cell_spell_reduce(torch.from_numpy(X).cuda(), RB, ROWS, 0.0, thr_d.to(torch.float16))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [5, 257, 1029])
def test_seasons(torch_cuda, dtype, n):
    """tests/test_gpu_spell.py's season case: open, null, ordinary and inverted windows, a day in no season, and cells 4..7 out of
    season together on row 6 -- the piece is not read and the runs end all the same.  Poison out of season changes nothing."""
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch = torch_cuda
    X = _field(n, dtype, seed=11 * n)
    X[:, 4:8] = 9.0
    doy = np.arange(100, 100 + T)
    doy[12] = 2000
    kinds = np.array([OPEN, 1 | 0 << 10 | WIN_NULL, 102 | 107 << 10, 103 | 105 << 10 | WIN_INVERT, 300 | 320 << 10], dtype=np.int32)
    win = kinds[np.arange(n) % 5]
    win[4:8] = 106 | 106 << 10 | WIN_INVERT
    thr = _thr(n, dtype, 2, 1, seed=n)
    thr[:, :, 4:8] = 5.0
    season = np.stack([in_season(int(doy[t]), win) for t in range(T)])
    poison = np.array([np.nan, np.inf, -np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 4]
    Xp = np.where(season, X, poison).astype(dtype)
    for pad in _pads(n, dtype):
        Xd, Xpd, thr_d = _strided(torch, X, pad), _strided(torch, Xp, pad), _dev_thr(torch, thr, pad_n=pad)
        for side in SIDES:
            for stat, L in (("days", 1), ("days", 3), ("events", 2), ("longest", 1), ("amount", 1)):
                kw = dict(min_length=L, stat=stat, side=side, doy=doy, windows=win)
                got, st = cell_spell_reduce(Xd, RB, ROWS, 0.0, thr_d, **kw)
                assert int(st.item()) == 0
                _same(got, cell_spell_ref(X, RB, ROWS, 0.0, thr, None, L, stat, side, doy, win), dtype, (n, pad, side, stat, L))
                g2, st = cell_spell_reduce(Xpd, RB, ROWS, 0.0, thr_d, **kw)
                assert torch.equal(g2, got) and int(st.item()) == 0
    longest = cell_spell_ref(X, RB, ROWS, 0.0, thr, None, 1, "longest", "above", doy, win)[0]
    if n > 5:
        assert longest[:, 4].tolist() == [4, 5, 0]                                        # rows 0-3, 5, 7-9 | 10 11, 13-17


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_public_call(torch_cuda, segment_plans, dtype, monkeypatch):
    """tas_relative_spell_aggregate on a small grid with a segment table, a Kelvin-shifted field, period="month" (31 days, then
    9) and twelve monthly planes of per-cell thresholds in degrees C: every statistic against the restatement aggregated by the
    fp64 oracle at the project's 1e-4 (fp32) / 1e-6 (fp64); cells="all" and "referenced"; a baseline from cell_quantiles of the
    same variable (offset exactly 0); 65 levels in two launches; results_on_device()."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import relative
    from climate_toolbox_amd.relative import CellThresholds, cell_quantiles
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, tas_relative_spell_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Sparse(16, 32, dtype, seed=29)
    Tn = c.T
    rb, rows = np.array([0, 31, Tn]), np.arange(Tn)
    flat = c.tas.reshape(Tn, c.G)
    rng = np.random.default_rng(5)
    levels = [0.9, 0.5, 0.99]
    planes12 = (6.85 + 12.0 * rng.standard_normal((3, 12, c.nlat, c.nlon)) + np.array([8.0, 0.0, 16.0])[:, None, None, None]).astype(dtype)
    th = CellThresholds.from_array(planes12, c.lat, c.lon, labels=np.arange(1, 13), levels=levels)
    ds = lambda device=True: convert_kelvin_to_celsius(c.dataset(torch, device=device), "tas")
    call = lambda t=th, d=None, **kw: tas_relative_spell_aggregate(d if d is not None else ds(), t, "popwt", "reg", c.df, period="month",
                                                                    planes="month", **kw)
    agg = lambda cells: np.stack([O.agg_coded(cells[k], c.cell, c.code, c.w_eff, c.R) for k in range(cells.shape[0])])

    def ok(got, want, cells, factor=1.0):
        """the project's bound: rtol relative to the oracle on |f| (the sums change sign between cells; counts are their own |f|)"""
        bound = agg(np.abs(np.nan_to_num(cells, nan=0.0)))
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        fin = ~np.isnan(want)
        assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= factor * c.rtol * bound[fin] + 1e-300).all()
    for stat, side, L in (("days", "above", 2), ("events", "above", 2), ("longest", "below", 3), ("amount", "above", 3), ("excess", "below", 1)):
        eff = L if stat in ("days", "events") else 1
        cells = cell_spell_ref(flat, rb, rows, -273.15, planes12.reshape(3, 12, c.G), [0, 1], eff, stat, side)
        assert len(np.unique(cells[~np.isnan(cells)])) > 2
        want = agg(cells)
        out = call(stat=stat, side=side, min_length=L)
        v = out["tas-relative-spell"]
        assert v.dims == ("threshold", "period", "reg") and v.attrs["stat"] == stat and v.attrs["side"] == side and v.attrs["min_length"] == eff
        assert v.attrs["units"] == {"days": "days", "longest": "days", "events": "1"}.get(stat, "C")
        assert list(out["threshold"].values) == levels and list(out["period"].values) == [200101, 200102]
        got = v.values
        assert isinstance(v.data, np.ndarray) and got.dtype == dtype and got.shape == (3, 2, c.R) and np.isnan(got[:, :, c.R - 1]).all()
        ok(got, want, cells)
        ref = call(stat=stat, side=side, min_length=L, cells="referenced")["tas-relative-spell"].values
        ok(ref, want, cells)
        ok(ref, got.astype(np.float64), cells, factor=2.0)                                # "all" equals "referenced", each within the bound
        np.testing.assert_array_equal(call(d=ds(device=False), stat=stat, side=side, min_length=L)["tas-relative-spell"].values, got)
    with pkg.results_on_device():
        on = call(stat=stat, side=side, min_length=L)
        assert isinstance(on["tas-relative-spell"].data, torch.Tensor) and on["tas-relative-spell"].data.is_cuda
    np.testing.assert_array_equal(on["tas-relative-spell"].values, got)
    # the baseline taken from the same Kelvin variable: raw elements against raw order statistics, TX90p per month
    base = cell_quantiles(ds(), [0.9], period="month", method="higher")
    assert base.shift == -273.15 and base.labels.tolist() == [200101, 200102] and tuple(base.values.shape) == (1, 2, c.nlat, c.nlon)
    tx = tas_relative_spell_aggregate(ds(), base, "popwt", "reg", c.df, period="month", min_length=1)["tas-relative-spell"].values
    valid = (~np.isnan(flat[:31])).sum(0), (~np.isnan(flat[31:])).sum(0)
    want = np.stack([O.agg_coded((m - np.ceil((m - 1) * 0.9)).astype(np.float64)[None, :], c.cell, c.code, c.w_eff, c.R)[0] for m in valid])
    _rel_ok(tx[0], want, c.rtol)
    # where the Kelvin shift sits: the excess does not care -- the baseline of the shifted variable gives the restatement in degrees C --
    # and the amount refuses shifted thresholds; against thresholds in final units, or on a variable without a shift, it is the sum
    base3 = cell_quantiles(ds(), [0.5, 0.9], period="month", method="linear")
    raw = base3.values.cpu().numpy().reshape(2, 2, c.G)                                   # raw (Kelvin) order statistics
    cells = cell_spell_ref(flat, rb, rows, 0.0, raw, None, 1, "excess", "above")          # (x - 273.15) - (thr - 273.15) = x - thr
    ex = tas_relative_spell_aggregate(ds(), base3, "popwt", "reg", c.df, period="month", stat="excess")["tas-relative-spell"]
    assert ex.attrs["units"] == "C" and np.nanmax(np.abs(cells)) > 1.0
    ok(ex.values, agg(cells), cells)
    with pytest.raises(ValueError, match="final units"):
        tas_relative_spell_aggregate(ds(), base3, "popwt", "reg", c.df, period="month", stat="amount")
    celsius = CellThresholds.from_array((raw.astype(np.float64) - 273.15).astype(dtype).reshape(2, 2, c.nlat, c.nlon), c.lat, c.lon,
                                        labels=base3.labels, levels=[0.5, 0.9])
    cells = cell_spell_ref(flat, rb, rows, -273.15, (raw.astype(np.float64) - 273.15).astype(dtype), None, 1, "amount", "above")
    am = tas_relative_spell_aggregate(ds(), celsius, "popwt", "reg", c.df, period="month", stat="amount")["tas-relative-spell"].values
    ok(am, agg(cells), cells)                                                             # degrees C summed over the hot days
    plain_k = c.dataset(torch)                                                            # the same field, Kelvin, no shift
    base_k = cell_quantiles(plain_k, [0.5, 0.9], period="month")
    assert base_k.shift == 0.0 and torch.equal(base_k.values, base3.values)
    cells = cell_spell_ref(flat, rb, rows, 0.0, raw, None, 1, "amount", "above")
    am_k = tas_relative_spell_aggregate(plain_k, base_k, "popwt", "reg", c.df, period="month", stat="amount")["tas-relative-spell"].values
    ok(am_k, agg(cells), cells)                                                           # Kelvin summed over the hot days
    # a grid that does not match, a period without a plane
    with pytest.raises(ValueError, match="grid does not match"):
        call(CellThresholds.from_array(planes12[:, :, 1:], c.lat[1:], c.lon, labels=np.arange(1, 13)))
    with pytest.raises(ValueError, match="200101"):
        call(CellThresholds.from_array(planes12[:, 1:], c.lat, c.lon, labels=np.arange(2, 13)))
    # 65 levels: 64, then 1, joined in order
    many = np.concatenate([planes12[:1, :1] + dtype(0.25 * k) for k in range(65)])
    th65 = CellThresholds.from_array(many, c.lat, c.lon)
    ran, real = [], relative.cell_spell_reduce
    monkeypatch.setattr(relative, "cell_spell_reduce", lambda *a, **k: (ran.append(int(a[4].shape[0])), real(*a, **k))[1])
    one = lambda t: tas_relative_spell_aggregate(ds(), t, "popwt", "reg", c.df, period="year", min_length=2)["tas-relative-spell"].values
    v = one(th65)
    assert ran == [64, 1] and v.shape == (65, 1, c.R)
    np.testing.assert_array_equal(v[64:], one(CellThresholds.from_array(many[64:], c.lat, c.lon)))
    np.testing.assert_array_equal(v[:3], one(CellThresholds.from_array(many[:3], c.lat, c.lon)))
