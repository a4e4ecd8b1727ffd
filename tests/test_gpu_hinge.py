"""Hinge and restricted-cubic-spline totals on the GPU (run with -m gpu): wagg_hinge_reduce_* through engine.hinge_reduce against
a NumPy restatement on raw matrices, and tas_hinge_aggregate / tas_rcspline_aggregate on a segment-table plan with a whole-line
chunking against the daily oracle (oracle.ref_numpy.agg_coded) of the restated terms.

The restatement forms d = (x + off) - k in the ELEMENT TYPE by the kernel's two operations (offset and knot converted to the
element type first) and negates it for side "below"; everything after is fp64: the powers (by multiplication), the sums over a
period's rows, the tail combination (S_j + ca_j S_A) + cb_j S_B and the aggregation.  Agreement is |got - ref| <= RTOL * A with
RTOL32 / RTOL64 of tests/test_gpu_parity.py and A the same sums / aggregation of the absolute parts, sum|h_j| + |ca_j| sum h_A +
|cb_j| sum h_B -- the scale rule of tests/test_gpu_large_pitch.py.  The largest ratio |got - ref| / (RTOL * A) seen is printed."""
import numpy as np
import pytest

from tests.test_gpu_packed_totals import _Sparse, _rel, segment_plans  # noqa: F401
from tests.test_gpu_parity import RTOL32, RTOL64
from tests.test_gpu_periods import _psum
from tests.test_gpu_seasons import KELVIN, _mask_TG, _mixed_cells, _pack, _seasons_for
from tests.test_hinge_host import rcspline_coefficients
from tests.test_seasons_host import ref_mask

pytestmark = pytest.mark.gpu

T = 80
TAIL_KNOTS = (21.5, 29.0)
ALL_YEAR = 0 | 1023 << 10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _terms(X, offset, knots, power, side):
    """(len(knots),) + X.shape daily terms in fp64: d in X's dtype by the kernel's two operations, the rest in fp64; NaN gives 0"""
    dt = X.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        xo = X + dt(offset)
        out = []
        for k in knots:
            d = xo - dt(k)
            d = (-d if side == "below" else d).astype(np.float64)
            t = d.copy()
            for _ in range(power - 1):
                t = t * d
            out.append(np.where(d > 0, t, 0.0))
    return np.stack(out)


class _Worst:
    def __init__(self):
        self.ratio = 0.0

    def close(self, got, ref, scale, rtol, what):
        got = (got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)).astype(np.float64)
        ref, scale = np.asarray(ref, dtype=np.float64), np.asarray(scale, dtype=np.float64)
        assert got.shape == ref.shape == scale.shape, (what, got.shape, ref.shape, scale.shape)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=str(what))
        fin = np.isfinite(ref)
        err, lim = np.abs(got[fin] - ref[fin]), rtol * scale[fin]
        if err.size:
            self.ratio = max(self.ratio, float((err / np.maximum(lim, 1e-300)).max()))
        bad = err > lim + 1e-300
        assert not bad.any(), "%r: %d of %d beyond RTOL * A, worst ratio %.3g" % (what, bad.sum(), bad.size, (err / np.maximum(lim, 1e-300)).max())


def _layouts(torch, X, V):
    """(name, device view of X): rows in 16-byte pieces; an odd row stride; a base pointer one element past an aligned address --
    the last two take the VEC = 1 instances"""
    tdt = torch.float32 if X.dtype == np.float32 else torch.float64
    n = X.shape[1]
    out = []
    for name, ld, shift in (("wide", (n + V - 1) // V * V, 0), ("odd ldx", n if n % 2 else n + 1, 0), ("offset base", (n + V) // V * V, 1)):
        buf = torch.zeros(X.shape[0] * ld + 16, dtype=tdt, device="cuda")
        view = buf[shift:shift + X.shape[0] * ld].view(X.shape[0], ld)[:, :n]
        view.copy_(torch.from_numpy(X).cuda())
        assert view.stride(0) == ld and (view.data_ptr() % 16 == 0) == (shift == 0)
        assert (name == "wide") == (ld % V == 0 and shift == 0)
        out.append((name, view))
    return out


@pytest.mark.parametrize("dtype,n,rtol", [(np.float32, 1027, RTOL32), (np.float64, 515, RTOL64)])
def test_kernel_equals_the_restatement(torch_cuda, dtype, n, rtol):
    """n = one full column block of 16-byte pieces plus a ragged piece.  T = 80 rows: one period of all of them is a SPLIT list
    (asserted from the workspace size); beside it three periods with an empty one, dropped rows and lists not in time order.
    64 knots (-38 .. 52 C on a Kelvin field, offset -273.15) for power 1 above, with and without the tail, on all three layouts, both lists, with mixed
    windows (all-year, null, empty, single-day, plain, inverted) and without a season; the other powers and side on the wide
    layout with the split list and on the odd stride with the three periods.  1, 8, 9 and 17 knots (one knot; a full group; a
    full group and one; two and one) are bit for bit the planes of the 64-knot call, with and without the tail; two runs are
    bit-equal; all-year windows give the bits of the call without a season.  A NaN cell totals 0; NaN, +-inf and 1e30 out of
    season change no bit and no status; an in-season +inf or -inf sets bit 0."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    L = _lib.load()
    V = 16 // np.dtype(dtype).itemsize
    rng = np.random.default_rng(n)
    X = (280 + 15 * rng.standard_normal((T, n))).astype(dtype)
    X[:, 6] = np.nan                                                              # (cell 6 is open all year)
    X[3, 0] = np.nan
    knots = np.concatenate([[-38.0, 52.0], rng.permutation(np.linspace(-20.0, 41.5, 62))])      # not sorted
    assert len(knots) == 64 == _lib.HINGE_MAX and _lib.HINGE_GROUP == 8
    ca, cb = rng.uniform(-3, 3, 64), rng.uniform(-3, 3, 64)
    tail = (TAIL_KNOTS, ca, cb)
    doy = np.arange(100, 100 + T)
    z1, z2 = _mixed_cells(n, doy)
    win = _pack(z1, z2)
    m01 = np.nan_to_num(ref_mask(z1, z2, doy), nan=0.0).T                         # (T, n)
    kinds = {int(w) >> 20 for w in win}
    assert (m01[:, 0] == 1).all() and kinds >= {0, 1, 2} and 0 < m01.mean() < 1   # plain, inverted and null windows
    one = (np.array([0, T]), np.arange(T))
    keep = np.flatnonzero(np.arange(T) % 5 != 2)                                  # dropped rows
    three = (np.array([0, 30, 30, len(keep)]), np.concatenate([rng.permutation(keep[:30]), rng.permutation(keep[30:])]))   # (not in time order)
    # the split: the workspace the library asks for holds `split` parts of 64 planes x 1 period x n fp64 sums
    wb = L.wagg_hinge_work_bytes(n, 1, T, 64)
    split = wb // (8 * 64 * 1 * n)
    assert split > 1 and wb == split * 8 * 64 * n
    layouts = _layouts(torch, X, V)
    worst = _Worst()

    daily = {}                                                                    # (power, side) -> the 64 + 2 daily term planes, computed once

    def reference(power, side, rb, rows, m, with_tail):
        """(the totals, A): every term is >= 0, so without the tail A is the total itself"""
        if (power, side) not in daily:
            daily.clear()
            daily[(power, side)] = _terms(X, KELVIN, np.concatenate([knots, TAIL_KNOTS]), power, side)
        sums = np.stack([_psum(p * m, rb, rows) for p in daily[(power, side)]])
        ref, hA, hB = sums[:64], sums[64], sums[65]
        if not with_tail:
            return ref, ref
        a, b = ca[:, None, None], cb[:, None, None]
        return (ref + a * hA) + b * hB, ref + np.abs(a) * hA + np.abs(b) * hB

    def run(Xd, lists, power, side, season, with_tail, sel=slice(None)):
        kw = {"doy": doy, "windows": win} if season else {}
        part = (TAIL_KNOTS, ca[sel], cb[sel]) if with_tail else None
        return engine.hinge_reduce(Xd, lists[0], lists[1], KELVIN, knots[sel], power=power, side=side, tail=part, **kw)

    wide = layouts[0][1]
    for power in (1, 2, 3):
        for side in ("above", "below"):
            full = power == 1 and side == "above"
            for with_tail in (False, True):
                for li, (lname, Xd) in enumerate(layouts):
                    for lists in (one, three):
                        for season in (True, False):
                            if not full and (li, lists is one, season) not in ((0, True, True), (1, False, False)):
                                continue
                            what = (power, side, with_tail, lname, "one" if lists is one else "three", season)
                            got, st = run(Xd, lists, power, side, season, with_tail)
                            assert got.shape == (64, len(lists[0]) - 1, n) and int(st.item()) == 0, what
                            ref, A = reference(power, side, lists[0], lists[1], m01 if season else np.ones_like(m01), with_tail)
                            worst.close(got, ref, A, rtol, what)
                            assert (got[:, :, 6] == 0).all(), what                # the NaN cell totals 0
                            if lists is three:
                                assert (got[:, 1] == 0).all(), what               # the empty period
                # fewer knots: other group counts, a ragged last group -- bit for bit the planes of the 64
                got, _ = run(wide, one, power, side, True, with_tail)
                again, _ = run(wide, one, power, side, True, with_tail)
                assert torch.equal(again, got)
                for sel in (slice(0, 1), slice(8, 9), slice(63, 64), slice(5, 13), slice(3, 12), slice(40, 57)):
                    part, st = run(wide, one, power, side, True, with_tail, sel)
                    assert torch.equal(part, got[sel]) and int(st.item()) == 0, (power, side, with_tail, sel)
    # an all-year window for every cell: the bits of the call without a season (both lists, tail and none, VEC wide and 1)
    every = np.full(n, ALL_YEAR, dtype=np.int32)
    for lname, Xd in layouts[:2]:
        for lists in (one, three):
            for with_tail in (False, True):
                part = tail if with_tail else None
                a, _ = engine.hinge_reduce(Xd, lists[0], lists[1], KELVIN, knots, power=3, tail=part, doy=doy, windows=every)
                b, _ = engine.hinge_reduce(Xd, lists[0], lists[1], KELVIN, knots, power=3, tail=part)
                assert torch.equal(a, b), (lname, with_tail)
    # whatever stands out of season is never looked at
    Xp = X.copy()
    poison = np.array([np.nan, np.inf, -np.inf, 1e30], dtype=dtype)[(np.arange(T)[:, None] + np.arange(n)[None, :]) % 4]
    Xp[m01 == 0] = poison[m01 == 0]
    for (lname, Xd), (_, Xq) in zip(layouts, _layouts(torch, Xp, V)):
        for side in ("above", "below"):
            a, sa = engine.hinge_reduce(Xd, one[0], one[1], KELVIN, knots[:9], power=2, side=side, doy=doy, windows=win)
            b, sb = engine.hinge_reduce(Xq, one[0], one[1], KELVIN, knots[:9], power=2, side=side, doy=doy, windows=win)
            assert torch.equal(a, b) and int(sa.item()) == 0 and int(sb.item()) == 0, lname
    # an in-season infinity (cells 12 and 18 are open all year) sets bit 0, whichever side is asked for, with and without a season
    for j, v in ((12, np.inf), (18, -np.inf)):
        Xi = X.copy()
        Xi[5, j] = v
        for lname, Xd in _layouts(torch, Xi, V)[:2]:
            for side in ("above", "below"):
                for kw in ({"doy": doy, "windows": win}, {}):
                    got, st = engine.hinge_reduce(Xd, three[0], three[1], KELVIN, knots[:3], side=side, **kw)
                    assert int(st.item()) == 1, (lname, v, side)
                    counted = (v > 0) == (side == "above")                        # +inf above / -inf below: the total is +inf
                    assert bool(torch.isinf(got[:, 0, j]).all()) == counted and bool(torch.isfinite(got[:, 2, j]).all())
    print("hinge kernel %s n = %d: largest |got - ref| / (RTOL * A) = %.3g" % (np.dtype(dtype).name, n, worst.ratio))


def test_binding_refuses_what_the_library_would(torch_cuda):
    from climate_toolbox_amd import engine
    torch = torch_cuda
    Xd = torch.zeros((9, 63), dtype=torch.float32, device="cuda")
    rb, rows = [0, 9], np.arange(9)
    for kw, text in (({"knots": []}, "knots"), ({"knots": list(range(65))}, "knots"), ({"knots": [0.0, float("nan")]}, "finite"),
                     ({"power": 0}, "power"), ({"power": 4}, "power"), ({"side": "over"}, "side"),
                     ({"tail": ((1.0, 2.0), [0.5], [0.5, 0.5])}, "tail"), ({"tail": ((1.0,), [0.5], [0.5])}, "tail"),
                     ({"tail": ((1.0, float("inf")), [0.5], [0.5])}, "tail"), ({"doy": np.arange(1, 10)}, "go together")):
        args = dict({"knots": [1.0]}, **kw)
        with pytest.raises(ValueError, match=text):
            engine.hinge_reduce(Xd, rb, rows, 0.0, args.pop("knots"), **args)
    got, st = engine.hinge_reduce(Xd + 3.0, rb, rows, -1.0, [0.5, 1.5], power=2)  # (3 - 1 - k)^2 on nine days
    assert got[:, 0, 7].tolist() == [9 * 1.5 ** 2, 9 * 0.5 ** 2] and int(st.item()) == 0


HINGE_KNOTS = [18.0, -4.5, 7.25, 26.0, 11.0]
SPLINE_KNOTS = [-8.0, 2.5, 9.0, 17.5, 27.0]


@pytest.mark.parametrize("dtype,kelvin", [(np.float32, True), (np.float64, False)])
def test_public_calls_match_the_oracle(torch_cuda, segment_plans, dtype, kelvin):
    """24 x 44 cells, 40 days of February and March 2004 (29 February among them), a segment-table plan with a whole-line
    chunking; an fp32 Kelvin field shifted by convert_kelvin_to_celsius (the shift is the kernel's offset) and an fp64 field in
    degrees C.  tas_hinge_aggregate (power 1 below, power 3 above) and tas_rcspline_aggregate (plain and normalised) with
    period="year" and "month", with and without a season, against the daily oracle of the restated terms; dims, coordinates and
    attributes; cells="referenced" packs and meets the same oracle (its difference to "all" is printed); the (lat, lon, time)
    layout, a host-resident field and results_on_device() give the bits of the plain call; leap_days="drop" is
    remove_leap_days first; 70 knots run in two launches and equal the two halves.  Cross-checks against existing code: cooling
    minus heating degree days at one knot k is the tas_poly power-1 total minus k times the counted days (tas_bins_aggregate
    with one open bin), and the spline is the host combination of tas_hinge_aggregate(power=3) at its knots."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, minixr, periods
    from climate_toolbox_amd.transformations import (convert_kelvin_to_celsius, remove_leap_days, tas_bins_aggregate, tas_hinge_aggregate,
                                                     tas_poly_aggregate, tas_rcspline_aggregate)
    torch = torch_cuda
    c = _Sparse(24, 44, dtype, seed=31)
    c.time = np.datetime64("2004-02-05") + np.arange(c.T)
    if not kelvin:
        c.tas = (c.tas.astype(np.float64) + KELVIN).astype(dtype)
    off = KELVIN if kelvin else 0.0
    rtol = RTOL32 if dtype == np.float32 else RTOL64
    gd, z1, z2 = _seasons_for(c, seed=c.T)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time))
    assert np.isnan(mask).any() and (mask == 0).any() and (mask == 1).any()
    flat = c.tas.reshape(c.T, c.G)
    worst = _Worst()
    packs = lambda: engine.PACK_STATS["device"] + engine.PACK_STATS["host"] + engine.PACK_STATS["host_fallback"]
    assert c.plan().compact_cells(dtype) is not None

    def dataset(device=True, moved=False, tas=None):
        f = c.tas if tas is None else tas
        if not moved:
            ds = c.dataset(torch, device=device, tas=f)
        else:
            wrap = (lambda v: torch.from_numpy(v).cuda()) if device else (lambda v: v)
            ds = minixr.Dataset({"tas": (("lat", "lon", "time"), wrap(np.ascontiguousarray(np.moveaxis(f, 0, -1))))},
                                coords={"time": c.time, "lat": c.lat, "lon": c.lon})
        ds["tas"].attrs["units"] = "K" if kelvin else "C"
        return convert_kelvin_to_celsius(ds, "tas") if kelvin else ds

    def oracle(daily, rb, rows, m):
        """period totals of the aggregated daily terms (n_planes, T, G) under the 0/1 mask m"""
        return np.stack([c.oracle(np.where(m == 1, d, 0.0), rb, rows)[0] for d in daily])

    hinge = lambda ds, knots=HINGE_KNOTS, **kw: tas_hinge_aggregate(ds, knots, "popwt", "reg", c.df, **kw)
    spline = lambda ds, **kw: tas_rcspline_aggregate(ds, SPLINE_KNOTS, "popwt", "reg", c.df, **kw)
    sca, scb = rcspline_coefficients(SPLINE_KNOTS)
    cubes = _terms(flat, off, SPLINE_KNOTS, 3, "above")                           # (5, T, G)
    every = np.ones_like(mask)
    kept = {}
    for period in ("year", "month"):
        labels, rb, rows = periods.period_rows(c.time, period)
        assert len(labels) == (1 if period == "year" else 2)
        for season, m in ((None, every), (sw, mask)):
            for power, side in ((1, "below"), (3, "above")):
                out = hinge(dataset(), power=power, side=side, period=period, season=season)
                v = out["tas-hinge"]
                assert v.dims == ("knot", "period", "reg") and v.attrs["side"] == side
                assert v.attrs["units"] == ("degreedays_C" if power == 1 else "C^3")
                assert out["knot"].values.dtype == np.float64 and list(out["knot"].values) == HINGE_KNOTS
                np.testing.assert_array_equal(out["period"].values, labels)
                got = v.values
                assert isinstance(v.data, np.ndarray) and got.dtype == dtype and got.shape == (5, len(labels), c.R)
                ref = oracle(_terms(flat, off, HINGE_KNOTS, power, side), rb, rows, m)
                assert np.isnan(ref[:, :, c.R - 1]).all() and np.isfinite(ref[:, :, :c.R - 1]).all()
                worst.close(got, ref, ref, rtol, (period, season is not None, power, side))
                kept[(period, season is not None, power, side)] = got
            for normalize in (False, True):
                out = spline(dataset(), period=period, season=season, normalize=normalize)
                v = out["tas-rcspline"]
                assert v.dims == ("term", "period", "reg") and v.attrs["units"] == "C^3"
                assert v.attrs["knots"] == ", ".join(repr(float(t)) for t in SPLINE_KNOTS) and "side" not in v.attrs
                assert list(out["term"].values) == SPLINE_KNOTS[:-2] and v.values.dtype == dtype
                H = oracle(cubes, rb, rows, m)
                ref = (H[:3] + sca[:, None, None] * H[3]) + scb[:, None, None] * H[4]
                A = H[:3] + np.abs(sca)[:, None, None] * H[3] + np.abs(scb)[:, None, None] * H[4]
                scale = (SPLINE_KNOTS[-1] - SPLINE_KNOTS[0]) ** 2 if normalize else 1.0
                worst.close(v.values, ref / scale, A / scale, rtol, (period, season is not None, "spline", normalize))
                if not normalize:
                    kept[(period, season is not None, "spline")] = v.values
                    # the spline is the host combination of the cubes tas_hinge_aggregate gives at its knots
                    Hg = hinge(dataset(), SPLINE_KNOTS, power=3, period=period, season=season)["tas-hinge"].values.astype(np.float64)
                    worst.close(v.values, (Hg[:3] + sca[:, None, None] * Hg[3]) + scb[:, None, None] * Hg[4], A, rtol,
                                (period, season is not None, "spline from hinges"))
    # cells="referenced": packs, meets the same oracle; the difference to "all" is printed
    labels, rb, rows = periods.period_rows(c.time, "month")
    for season, m in ((None, every), (sw, mask)):
        n0 = packs()
        got = hinge(dataset(), power=3, side="above", period="month", season=season, cells="referenced")["tas-hinge"].values
        sp = spline(dataset(), period="month", season=season, cells="referenced")["tas-rcspline"].values
        assert packs() >= n0 + 2
        n0 = packs()
        old, old_sp = kept[("month", season is not None, 3, "above")], kept[("month", season is not None, "spline")]
        print("24x44 %s%s: referenced vs all, max rel diff hinge %.3g, spline %.3g" % (np.dtype(dtype).name, ", season" if season is not None else "",
                                                                                    _rel(got, old), _rel(sp, old_sp)))
        ref = oracle(_terms(flat, off, HINGE_KNOTS, 3, "above"), rb, rows, m)
        worst.close(got, ref, ref, rtol, ("referenced", season is not None))
        H = oracle(cubes, rb, rows, m)
        worst.close(sp, (H[:3] + sca[:, None, None] * H[3]) + scb[:, None, None] * H[4],
                    H[:3] + np.abs(sca)[:, None, None] * H[3] + np.abs(scb)[:, None, None] * H[4], rtol, ("referenced spline", season is not None))
        np.testing.assert_array_equal(spline(dataset(device=False), period="month", season=season, cells="referenced")["tas-rcspline"].values, sp)
    # other layouts and residencies: the same kernels on the same numbers
    kw = dict(period="month", season=sw)
    base = kept[("month", True, "spline")]
    np.testing.assert_array_equal(spline(dataset(device=False), **kw)["tas-rcspline"].values, base)
    moved = spline(dataset(moved=True), **kw)
    assert moved["tas-rcspline"].dims == ("term", "reg", "period")
    np.testing.assert_array_equal(np.swapaxes(moved["tas-rcspline"].values, 1, 2), base)
    np.testing.assert_array_equal(np.swapaxes(hinge(dataset(device=False, moved=True), power=3, **kw)["tas-hinge"].values, 1, 2),
                                  kept[("month", True, 3, "above")])
    with pkg.results_on_device():
        on = spline(dataset(), normalize=True, **kw)
        assert isinstance(on["tas-rcspline"].data, torch.Tensor) and on["tas-rcspline"].data.is_cuda
        assert isinstance(hinge(dataset(device=False), **kw)["tas-hinge"].data, np.ndarray)    # (a host-resident field's: a host array)
        on_h = hinge(dataset(), power=3, **kw)
        assert on_h["tas-hinge"].data.is_cuda
    np.testing.assert_array_equal(on_h["tas-hinge"].values, kept[("month", True, 3, "above")])
    np.testing.assert_array_equal(on["tas-rcspline"].values, spline(dataset(), normalize=True, **kw)["tas-rcspline"].values)
    # leap days: "drop" is remove_leap_days first; "keep" counts 29 February like any day
    dropped = hinge(dataset(), period="year", leap_days="drop")["tas-hinge"].values
    np.testing.assert_array_equal(dropped, hinge(remove_leap_days(dataset()), period="year")["tas-hinge"].values)
    assert (c.time == np.datetime64("2004-02-29")).any() and not np.array_equal(dropped, hinge(dataset(), period="year")["tas-hinge"].values,
                                                                                equal_nan=True)
    # 70 knots: 64, then 6, joined in order -- the two halves called separately, bit for bit
    many = list(np.linspace(-25.0, 44.0, 70))
    ran, real = [], engine.hinge_reduce
    engine.hinge_reduce = lambda *a, **k: (ran.append(len(a[4])), real(*a, **k))[1]
    try:
        out = hinge(dataset(), many, power=2, **kw)
    finally:
        engine.hinge_reduce = real
    assert ran == [64, 6] and list(out["knot"].values) == many and out["tas-hinge"].values.shape == (70, 2, c.R)
    np.testing.assert_array_equal(out["tas-hinge"].values[:64], hinge(dataset(), many[:64], power=2, **kw)["tas-hinge"].values)
    np.testing.assert_array_equal(out["tas-hinge"].values[64:], hinge(dataset(), many[64:], power=2, **kw)["tas-hinge"].values)
    # cooling - heating degree days at k = sum over the counted days of (x - k) = the tas_poly power-1 total - k * counted days.
    # tas_poly works on the 365-day calendar, numbers the days from 1 and takes its field to be in kelvin: so leap_days="drop"
    # and a label per remaining day on this side, no season, and for the field in degrees C the knot as tas_poly sees it is
    # k - 273.15.
    k = 11.0
    stays = c.time != np.datetime64("2004-02-29")
    lab = (c.time[stays].astype("datetime64[M]") - np.datetime64("2004-01")).astype(np.int64)
    _, rb_d, rows_d = periods.period_rows(c.time[stays], lab)
    sub = _Sparse.__new__(_Sparse)
    sub.__dict__.update(c.__dict__, T=c.T - 1)
    kw2 = dict(period=lab, leap_days="drop")
    cdd = hinge(dataset(), [k], side="above", **kw2)["tas-hinge"].values.astype(np.float64)[0]
    hdd = hinge(dataset(), [k], side="below", **kw2)["tas-hinge"].values.astype(np.float64)[0]
    poly = tas_poly_aggregate(c.dataset(torch, tas=c.tas), [1], "popwt", "reg", c.df, period=lab)["tas-poly-1"].values.astype(np.float64)
    days = tas_bins_aggregate(dataset(), [-np.inf, np.inf], "popwt", "reg", c.df, **kw2)["tas-bins"].values.astype(np.float64)[0]
    assert cdd.shape == hdd.shape == poly.shape == days.shape == (2, c.R)
    both = _terms(flat[stays], off, [k], 1, "above")[0] + _terms(flat[stays], off, [k], 1, "below")[0]
    worst.close(cdd - hdd, poly - (k if kelvin else k + KELVIN) * days, sub.oracle(both, rb_d, rows_d)[0], rtol, "cooling - heating")
    print("hinge public calls %s: largest |got - ref| / (RTOL * A) = %.3g" % (np.dtype(dtype).name, worst.ratio))


def test_counted_inf_raises(torch_cuda, segment_plans):
    """+-inf out of season is nobody's business; counted, it raises ValueError from both calls -- with and without a season.  NaN
    counts 0 and raises nothing."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd.transformations import tas_hinge_aggregate, tas_rcspline_aggregate
    torch = torch_cuda
    c = _Sparse(24, 44, np.float32, seed=5)
    gd, z1, z2 = _seasons_for(c, seed=8)
    sw = pkg.season_windows(gd)
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time)).reshape(c.T, c.nlat, c.nlon)
    referenced = np.zeros(c.G, dtype=bool)
    referenced[c.cell] = True
    referenced = np.broadcast_to(referenced.reshape(1, c.nlat, c.nlon), mask.shape)
    calls = (lambda season: tas_hinge_aggregate(c.dataset(torch), [280.0, 290.0], "popwt", "reg", c.df, side="below", season=season)["tas-hinge"].values,
             lambda season: tas_rcspline_aggregate(c.dataset(torch), [270.0, 280.0, 290.0], "popwt", "reg", c.df, season=season)["tas-rcspline"].values)
    for call in calls:
        clean = call(sw)
        t, i, j = [int(v[0]) for v in np.nonzero((mask == 0) & referenced)]
        keep = c.tas[t, i, j]
        c.tas[t, i, j] = np.inf
        np.testing.assert_array_equal(call(sw), clean)
        with pytest.raises(ValueError, match="inf"):
            call(None)
        c.tas[t, i, j] = keep
        t, i, j = [int(v[0]) for v in np.nonzero((mask == 1) & referenced)]
        keep = c.tas[t, i, j]
        c.tas[t, i, j] = -np.inf
        with pytest.raises(ValueError, match="inf"):
            call(sw)
        c.tas[t, i, j] = np.nan
        assert np.isfinite(call(sw)[:, :, :c.R - 1]).all()
        c.tas[t, i, j] = keep
