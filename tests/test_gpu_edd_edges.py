"""Snyder degree days element by element on every kernel that evaluates them (run with -m gpu): the catalogue of
tests/edd_edges.py laid out as ``field[t, g] = case[(g + 7 t) mod E]`` and read back through a table of one segment per
region (R = G, a fixed permutation, weight 1), so that ``out[t, code[g]]`` IS the element -- no average to hide behind.

On every route: (a) NaN positions -- through an aggregation the zeros S6 makes of them -- and +-inf equal the reference's;
(b) the elements the reference SELECTS (M - e where tasmin >= e, 0 where tasmax <= e) agree bit for bit; (c) in-band elements
are within the derived ``edd_edges.bound`` of the form that route documents for that dtype and item; (d) in band
``got >= 0`` and ``got >= max(M - e, 0) - bound``.  (e) The split form of fp32 full-form dense plans is exempt from (b) and gets
the documented split bound (tests/test_gpu_dense_split.py::_bound) added to (c).  (f) Where the project documents bit equality
it is asserted on this field too: a second apply, the (R, T) result, host against device, ladder planes against the
four-plane kernels.  Each test prints its largest error / bound."""
import functools

import numpy as np
import pytest

from tests import edd_edges as EE
from tests.test_gpu_dense_split import _bound as split_bound

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
GRIDS = [(16, 64), (12, 80)]                     # G = 1024: whole 128-byte lines; G = 960: row_len no multiple of 32 or 16
TS = [70, 3]                                     # one full 64-timestep item plus a tail of 6; a tail alone
SHAPES = [(d, g, T) for d in DTYPES for g in GRIDS for T in TS]
SHAPE_IDS = ["%s-%dx%d-T%d" % ("f32" if d == np.float32 else "f64", g[0], g[1], T) for d, g, T in SHAPES]
PLANT_T = (1, 65)                                # one NaN tasmin in every 8th cell of these rows: every item holds one
LADDER = [-400.0, -1.75, 8.0, 29.0, 30.3, 303.15, 20.0, 1000.0, 12.5]      # 9: crosses the group of 8; -400 / 1000: whole
                                                                           # waves outside the band; 20 / 12.5: mostly inside


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _form(dtype, finite_item=False):
    """the evaluation a route documents (csrc/wagg_common.h): fp32 is the cheap form everywhere; fp64 the degree-13 fit in
    the loader/consumer kernel's finite items and libm everywhere else"""
    if dtype == np.float32:
        return "fit32"
    return "fit64" if finite_item else "libm"


@functools.lru_cache(maxsize=None)
def _code(G):
    c = np.random.default_rng(G).permutation(G).astype(np.int32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _planted(T, G):
    m = np.zeros((T, G), bool)
    for t in PLANT_T:
        if t < T:
            m[t, 3::8] = True
    return m


@functools.lru_cache(maxsize=None)
def _fields(dtype, kelvin, which, grid, T, plant):
    """(tasmin, tasmax) as (T, G) host arrays, left unchanged"""
    G = grid[0] * grid[1]
    lo, hi = EE.pool(dtype, kelvin, which)
    idx = EE.field_index(T, G, len(lo))
    lo, hi = lo[idx], hi[idx]
    if plant:
        lo[_planted(T, G)] = np.nan
    lo.setflags(write=False), hi.setflags(write=False)
    return lo, hi


class _Exp:
    pass


@functools.lru_cache(maxsize=None)
def _expect(dtype, kelvin, which, grid, T, plant, e):
    """what the reference gives on that field at threshold ``e``, computed once per case and spread over the field"""
    G = grid[0] * grid[1]
    lo, hi = EE.pool(dtype, kelvin, which)
    off = EE.KELVIN if kelvin else 0.0
    idx = EE.field_index(T, G, len(lo))
    x = _Exp()
    outer, vals = EE.exact_outer(lo, hi, off, e, dtype)
    x.ref, x.outer, x.vals, x.band = EE.reference(lo, hi, off, e, dtype)[idx], outer[idx], vals[idx], EE.in_band(lo, hi, off, e, dtype)[idx]
    x.ylo, x.yhi = EE.moved(lo, off, dtype)[idx], EE.moved(hi, off, dtype)[idx]
    if plant:
        p = _planted(T, G)
        x.ref[p], x.outer[p], x.band[p] = np.nan, False, False
    x.e = e
    x.floor = np.zeros(x.ref.shape)                               # max(M - e, 0) in band
    b = x.band
    x.floor[b] = np.maximum((x.yhi[b].astype(np.float64) + x.ylo[b]) / 2 - float(dtype(e)), 0.0)
    for a in (x.ref, x.outer, x.vals, x.band, x.floor):
        a.setflags(write=False)
    return x


def _check(got, x, dtype, form, aggregated, what, extra=None, exact=True):
    """assertions (a) - (d) of the module's docstring on one (T, G) plane; returns max error / bound over the band"""
    assert got.dtype == dtype and got.shape == x.ref.shape, what
    nan, inf = np.isnan(x.ref), np.isinf(x.ref)
    if aggregated:
        assert not np.isnan(got).any() and (got[nan] == 0).all(), what          # (a) S6: NaN counts 0
    else:
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    np.testing.assert_array_equal(got[inf], x.ref[inf].astype(dtype), err_msg=what)
    assert not np.isinf(got[~inf]).any(), what
    if exact:                                                                   # (b) (== takes -0 for +0 and nothing else)
        bad = x.outer & (got != x.vals)
        assert not bad.any(), "%s: %d selected elements differ, e = %r, first (tasmin, tasmax, got, want) = %r" % (
            what, bad.sum(), x.e, (x.ylo[bad][0], x.yhi[bad][0], got[bad][0], x.vals[bad][0]))
    b = x.band
    bnd = EE.bound(x.ylo[b], x.yhi[b], x.e, dtype, form)
    if extra is not None:
        bnd = bnd + extra[b]
    err = np.abs(got[b].astype(np.longdouble) - x.ref[b]).astype(np.float64)
    ratio = float((err / bnd).max()) if b.any() else 0.0           # (a threshold outside all data has no band)
    print("%s e=%g %s: max error / bound = %.3f" % (what, x.e, form, ratio))
    assert ratio <= 1.0, "%s: in-band error %.3f of the bound, e = %r" % (what, ratio, x.e)                     # (c)
    assert (got[b] >= 0).all(), what                                                                              # (d)
    assert (got[b] >= x.floor[b] - bnd).all(), what
    return ratio


def _dev(torch, a, layout="TG"):
    return torch.from_numpy(np.ascontiguousarray(a if layout == "TG" else a.T)).cuda()


def _thr(kelvin):
    return list(EE.CELSIUS_THRESHOLDS) if kelvin else list(EE.THRESHOLDS)


# ---- engine.transform_edd (xform_edd_kernel) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,grid,T", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kelvin", [False, True], ids=["celsius", "kelvin"])
def test_transform_edd(torch_cuda, dtype, grid, T, kelvin):
    from climate_toolbox_amd import engine
    lo, hi = _fields(dtype, kelvin, "all", grid, T, False)
    off = EE.KELVIN if kelvin else 0.0
    lod, hid = _dev(torch_cuda, lo), _dev(torch_cuda, hi)
    thr = _thr(kelvin)
    for e in thr:
        got = engine.transform_edd(lod, hid, off, [(1.0, e)]).cpu().numpy().reshape(lo.shape)
        _check(got, _expect(dtype, kelvin, "all", grid, T, False, e), dtype, _form(dtype), False, "transform_edd")
    # three terms: s = 1 f(e0); s += -1 f(e1); s += 0.5 f(e2), in the data type (coefficients +-1 and 0.5: every product exact)
    coefs, es = (1.0, -1.0, 0.5), thr[1:4]
    xs = [_expect(dtype, kelvin, "all", grid, T, False, e) for e in es]
    got = engine.transform_edd(lod, hid, off, list(zip(coefs, es))).cpu().numpy().reshape(lo.shape)
    with np.errstate(invalid="ignore"):
        ref = sum(c * x.ref for c, x in zip(coefs, xs))
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        allsel = xs[0].outer & xs[1].outer & xs[2].outer
        want = ((dtype(1) * xs[0].vals + dtype(-1) * xs[1].vals).astype(dtype) + dtype(0.5) * xs[2].vals).astype(dtype)
        np.testing.assert_array_equal(got[allsel], want[allsel])
        fin = np.isfinite(ref) & ~allsel
        # every term's own bound (0 where it is selected) plus the two roundings of the sums
        u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
        bnd = np.zeros(ref.shape)
        for c, x in zip(coefs, xs):
            bk = np.zeros(ref.shape)
            bk[x.band] = EE.bound(x.ylo[x.band], x.yhi[x.band], x.e, dtype, _form(dtype))
            bnd += abs(c) * bk + 2 * u * abs(c) * np.abs(np.where(np.isfinite(x.ref), x.ref, 0)).astype(np.float64)
        err = np.abs(got[fin].astype(np.longdouble) - ref[fin]).astype(np.float64)
        assert fin.sum() > 100 and (err <= bnd[fin]).all()


# ---- the segment table: sparse_lcv_kernel<..., EDD> (finite items: the selection-free form), sparse_gather_kernel, host -------
class _Plans:
    def __init__(self):
        self.p = {}

    def get(self, grid, route):
        from climate_toolbox_amd import _lib, engine
        if (grid, route) not in self.p:
            G = grid[0] * grid[1]
            kw = dict(row_len=grid[1]) if route == "lcv" else dict(flags=_lib.PLAN_NO_LINES)
            self.p[(grid, route)] = engine.SparsePlan(np.arange(G, dtype=np.int32), _code(G), np.ones(G), G, G, **kw)
        return self.p[(grid, route)]

    def close(self):
        for p in self.p.values():
            p.close()


@pytest.fixture(scope="module")
def plans(torch_cuda):
    p = _Plans()
    yield p
    p.close()


def _sparse_route(torch, plan, dtype, grid, T, kelvin, which, plant, counts, finite_item, layouts, what):
    G = grid[0] * grid[1]
    code = _code(G)
    lo, hi = _fields(dtype, kelvin, which, grid, T, plant)
    off = EE.KELVIN if kelvin else 0.0
    thr = _thr(kelvin)
    host = None
    for n in counts:
        es = (thr * 2)[1:1 + n]                                    # (n = 5 in Kelvin: one threshold twice, in two passes)
        for lay in layouts:
            a, b = _dev(torch, lo, lay), _dev(torch, hi, lay)
            out = plan.apply_edd(a, b, es, offset=off, layout=lay)
            got = out.cpu().numpy()
            assert torch.equal(plan.apply_edd(a, b, es, offset=off, layout=lay), out), what            # (f) a second apply
            rt = plan.apply_edd(a, b, es, offset=off, layout=lay, out_layout="RT").cpu().numpy()
            np.testing.assert_array_equal(np.swapaxes(rt, 1, 2), got)                                  # (f) (R, T): transposed bits
            for k, e in enumerate(es):
                _check(got[k][:, code], _expect(dtype, kelvin, which, grid, T, plant, e), dtype, _form(dtype, finite_item), True,
                       "%s %s n=%d" % (what, lay, n))
            if lay == "TG":
                host = plan.apply_edd_host(lo, hi, es, offset=off)
                np.testing.assert_array_equal(host, got)                                               # (f) host equals device
    plan.status()
    assert host is not None


@pytest.mark.parametrize("dtype,grid,T", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kelvin", [False, True], ids=["celsius", "kelvin"])
def test_lcv_finite_items(torch_cuda, plans, dtype, grid, T, kelvin):
    """every loaded value finite: the consumers take snyder_edd1_finite, which must give the selected elements exactly"""
    _sparse_route(torch_cuda, plans.get(grid, "lcv"), dtype, grid, T, kelvin, "finite", False, (1, 3, 5), True, ("TG", "GT"), "lcv finite")


@pytest.mark.parametrize("dtype,grid,T", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kelvin", [False, True], ids=["celsius", "kelvin"])
def test_lcv_general_items(torch_cuda, plans, dtype, grid, T, kelvin):
    """a NaN in every item (and the catalogue's own NaN and +-inf cases): the general form, whose other elements must not
    depend on that"""
    _sparse_route(torch_cuda, plans.get(grid, "lcv"), dtype, grid, T, kelvin, "all", True, (1, 3, 5), False, ("TG", "GT"), "lcv general")


def test_lcv_same_bits_with_and_without_a_nan_in_the_item_where_selected(torch_cuda, plans):
    """the selected elements of a finite field do not change when a NaN elsewhere switches their item to the general form"""
    grid, T = GRIDS[0], 70
    G = grid[0] * grid[1]
    plan = plans.get(grid, "lcv")
    for dtype in DTYPES:
        lo, hi = _fields(dtype, False, "finite", grid, T, False)
        lo2 = lo.copy()
        lo2[_planted(T, G)] = np.nan
        es = list(EE.THRESHOLDS[:4])
        a = plan.apply_edd(_dev(torch_cuda, lo), _dev(torch_cuda, hi), es).cpu().numpy()
        b = plan.apply_edd(_dev(torch_cuda, lo2), _dev(torch_cuda, hi), es).cpu().numpy()
        for k, e in enumerate(es):
            x = _expect(dtype, False, "finite", grid, T, False, e)
            sel = x.outer & ~_planted(T, G)
            assert sel.sum() > 1000
            np.testing.assert_array_equal(a[k][:, _code(G)][sel], b[k][:, _code(G)][sel])


@pytest.mark.parametrize("dtype,grid,T", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kelvin", [False, True], ids=["celsius", "kelvin"])
def test_gather_kernel(torch_cuda, plans, dtype, grid, T, kelvin):
    plan = plans.get(grid, "gather")
    assert plan.info["lines"] == 0
    _sparse_route(torch_cuda, plan, dtype, grid, T, kelvin, "all", False, (1, 4), False, ("TG", "GT"), "gather")


# ---- the dense family ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,grid,T", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("form", ["full", "tiles", "entries"])
def test_dense_forms(torch_cuda, dtype, grid, T, form):
    """the packers (pack_xf) of the three forms; no +-inf here (saw_inf and the redo are tested elsewhere)"""
    from climate_toolbox_amd.engine import DensePlan
    torch = torch_cuda
    G = grid[0] * grid[1]
    code = _code(G)
    name = "float32" if dtype == np.float32 else "float64"
    plan = DensePlan.from_segments(np.arange(G, dtype=np.int32), code, np.ones(G), G, G, dtype=name, form=form)
    assert plan.info["form"] == {"full": 0, "tiles": 1, "entries": 2}[form]
    W = np.zeros((G, G), dtype)
    W[np.arange(G), code] = 1
    for kelvin in (False, True):
        lo, hi = _fields(dtype, kelvin, "nan", grid, T, False)
        off = EE.KELVIN if kelvin else 0.0
        lod, hid = _dev(torch, lo), _dev(torch, hi)
        for e in _thr(kelvin):
            x = _expect(dtype, kelvin, "nan", grid, T, False, e)
            what = "dense %s %s" % (form, "kelvin" if kelvin else "celsius")
            if dtype == np.float32 and form == "full":
                ex = plan.apply_edd(lod, hid, e, offset=off, exact=True)
                _check(ex.cpu().numpy()[:, code], x, dtype, _form(dtype), True, what + " exact")
                got = plan.apply_edd(lod, hid, e, offset=off)
                assert torch.equal(plan.apply_edd(lod, hid, e, offset=off), got)
                # (e) the split form: its documented bound on the transformed field, no bit equality
                X = np.where(np.isnan(x.ref), 0.0, x.ref).astype(np.float64)
                _check(got.cpu().numpy()[:, code], x, dtype, _form(dtype), True, what + " split", extra=split_bound(X, W)[:, code], exact=False)
                sel = x.outer
                assert np.all(np.abs(got.cpu().numpy()[:, code][sel].astype(np.float64) - x.vals[sel]) <= split_bound(X, W)[:, code][sel])
            else:
                got = plan.apply_edd(lod, hid, e, offset=off)
                assert torch.equal(plan.apply_edd(lod, hid, e, offset=off), got)
                _check(got.cpu().numpy()[:, code], x, dtype, _form(dtype), True, what)
    assert not plan.saw_inf()
    plan.close()


# ---- the row-list kernels: one-row periods, so out[k, p, j] is the element -----------------------------------------------------
@pytest.mark.parametrize("dtype,grid,T", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kelvin", [False, True], ids=["celsius", "kelvin"])
def test_rowlist_kernels(torch_cuda, dtype, grid, T, kelvin):
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    G = grid[0] * grid[1]
    lo, hi = _fields(dtype, kelvin, "all", grid, T, False)
    off = EE.KELVIN if kelvin else 0.0
    lod, hid = _dev(torch, lo), _dev(torch, hi)
    rb, rows = np.arange(T + 1), np.arange(T)
    thr = LADDER
    assert len(thr) == _lib.EDD_LADDER_GROUP + 1
    xs = [_expect(dtype, kelvin, "all", grid, T, False, e) for e in thr]
    form = _form(dtype)
    # period_reduce, four and one threshold at a time
    per = []
    for s in (slice(0, 4), slice(4, 8), slice(8, 9)):
        out, st = engine.period_reduce(lod, rb, rows, X2=hid, edd=(off, thr[s]))
        # status bit 0: a transformed value was +-inf (a selected M - e with tasmax = +inf over tasmin >= e)
        assert (int(st.item()) & 1) == int(any(np.isinf(x.ref).any() for x in xs[s]))
        per += list(out)
    assert any(np.isinf(x.ref).any() for x in xs)
    for k, x in enumerate(xs):
        _check(per[k].cpu().numpy(), x, dtype, form, True, "period_reduce")
    # the ladder without a season: plane k is the period kernel's, bit for bit -- the ballot shortcut included
    lad, st = engine.edd_ladder_reduce(lod, hid, rb, rows, off, thr)
    assert int(st.item()) & 1 and lad.shape == (len(thr), T, G)
    assert torch.equal(engine.edd_ladder_reduce(lod, hid, rb, rows, off, thr)[0], lad)
    for k, x in enumerate(xs):
        assert torch.equal(lad[k], per[k]), ("ladder plane against period_reduce", thr[k])
        _check(lad[k].cpu().numpy(), x, dtype, form, True, "edd_ladder_reduce")
    # seasons: a window open all year, and one that cuts T (first and last row out of season: exactly 0)
    doy = np.arange(100, 100 + T)
    for name, first, last in (("all year", 0, 1023), ("cut", 101, 100 + T - 2)):
        win = np.full(G, first | last << 10, dtype=np.int32)
        inside = (doy >= first) & (doy <= last)
        assert inside.all() == (name == "all year") and inside.any()
        sea = []
        for g in (thr[:4], thr[4:8], thr[8:]):
            out, st = engine.season_reduce(lod, rb, rows, doy, win, X2=hid, edd=(off, g))
            sea += list(out)
        lad_s, _ = engine.edd_ladder_reduce(lod, hid, rb, rows, off, thr, doy=doy, windows=win)
        for k, x in enumerate(xs):
            assert torch.equal(lad_s[k], sea[k]), ("ladder plane against season_reduce", name, thr[k])
            got = sea[k].cpu().numpy()
            assert (got[~inside] == 0).all()
            if name == "all year":
                assert torch.equal(sea[k], per[k])
                _check(got, x, dtype, form, True, "season_reduce all year")
            else:
                np.testing.assert_array_equal(got[inside], per[k].cpu().numpy()[inside])
