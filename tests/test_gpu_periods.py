"""Period totals on the GPU (run with -m gpu): wagg_period_reduce_* through engine.period_reduce, and
weighted_aggregate_grid_to_regions_periods on both routes (reduce-first, aggregate-first) and both plan kinds (segment
table, dense family), at the smallest shapes at which the kernel can go wrong.

Oracle: oracle.ref_numpy.agg_coded on the daily (transformed) field, then a plain fp64 np.sum over each period's rows (NaN
propagates).  Tolerances: the project's _rel_ok with RTOL64 / RTOL32, ``scale`` = the same oracle run on |f| (cancellation
between warm and cold days is not error)."""
import numpy as np
import pandas as pd
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok

pytestmark = pytest.mark.gpu

KELVIN = -273.15


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _psum(daily, rb, rows):
    """(T, ...) daily values -> (P, ...) plain fp64 sums over each period's rows"""
    daily = np.asarray(daily, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([daily[rows[rb[p]:rb[p + 1]]].sum(axis=0) for p in range(len(rb) - 1)]) if len(rb) > 1 \
            else np.zeros((0,) + daily.shape[1:])


def _ok(got, ref, rtol, absref):
    """_rel_ok with an elementwise scale: |got - ref| <= rtol * max(|ref|, the oracle on |f|)"""
    ref = np.asarray(ref, dtype=np.float64)
    _rel_ok(got, ref, rtol, scale=np.asarray(absref, dtype=np.float64)[np.isfinite(ref)])


# a sum of T <= 70 terms accumulated in fp64 (T * 2^-53 relative to sum |f|), rounded once to the element type
SUM_TOL = {np.float32: 2e-7, np.float64: 1e-13}


def _structures(T):
    """period label arrays of T rows: (name, labels)"""
    out = [("all", np.zeros(T, dtype=np.int64)), ("each", np.arange(T)), ("interleaved", np.arange(T) % 3)]
    if T >= 9:
        drop = np.arange(T) % 3
        drop[1::4] = -1
        out.append(("dropped", drop))
    if T == 70:
        out.append(("1/31/38", np.repeat([0, 1, 2], [1, 31, 38])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the kernel, through engine.period_reduce
# ---------------------------------------------------------------------------------------------------------------------
def _field(rng, T, n, pad, dtype, torch):
    """(T, n) field as a device tensor with row stride n + pad, and its host copy"""
    X = (280 + 15 * rng.standard_normal((T, n))).astype(dtype)
    buf = torch.zeros((T, n + pad), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(X).cuda()
    return buf[:, :n], X


@pytest.mark.parametrize("dtype,rtol", [(np.float32, RTOL32), (np.float64, RTOL64)])
@pytest.mark.parametrize("n,pad", [(63, 0), (63, 3), (256, 0), (1100, 0), (1100, 3)])
@pytest.mark.parametrize("T", [1, 9, 70])
def test_kernel_sums_match_numpy(torch_cuda, dtype, rtol, n, pad, T):
    """Plain sums, four powers and three degree-day thresholds in one call each; aligned rows (16-byte pieces, the last one
    partial: 63 and 1100 are no multiples of 4) and a row stride that breaks the alignment (scalar path); one block and
    several (n = 1100); lists long enough to be split across blocks (T = 70 with few periods) and not."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.periods import period_rows
    from oracle import ref_numpy as O
    torch = torch_cuda
    rng = np.random.default_rng(100 * T + n + pad)
    Xd, X = _field(rng, T, n, pad, dtype, torch)
    H = (X + rng.uniform(0, 12, X.shape)).astype(dtype)
    Hd = torch.zeros((T, n + pad), dtype=Xd.dtype, device="cuda")
    Hd[:, :n] = torch.from_numpy(H).cuda()
    Hd = Hd[:, :n]
    assert Xd.stride(0) == n + pad
    X[0, 0] = np.nan
    X[:, 5] = np.nan                                    # NaN on every day
    Xd.copy_(torch.from_numpy(X).cuda())
    thr = [float(X[0, 1] + dtype(KELVIN)), 12.5, float(H[0, 2] + dtype(KELVIN))]      # a cell's own tasmin and tasmax among them
    for name, lab in _structures(T):
        labels, rb, rows = period_rows(np.arange(T), lab)
        if name == "interleaved":                       # ... with an empty period in the middle
            rb = np.concatenate([rb[:1], rb[:1], rb[1:]])
        P = len(rb) - 1
        # plain sums: NaN counts 0 / NaN propagates
        got, st = engine.period_reduce(Xd, rb, rows)
        assert got.shape == (1, P, n) and int(st.item()) == 0
        _ok(got[0].cpu().numpy(), _psum(np.nan_to_num(X, nan=0.0), rb, rows), SUM_TOL[dtype],
            _psum(np.abs(np.nan_to_num(X, nan=0.0)), rb, rows))
        keep, _ = engine.period_reduce(Xd, rb, rows, keep_nan=True)
        _ok(keep[0].cpu().numpy(), _psum(X, rb, rows), SUM_TOL[dtype], _psum(np.abs(np.nan_to_num(X, nan=0.0)), rb, rows))
        if name == "interleaved":
            assert (got[0, 0] == 0).all() and (keep[0, 0] == 0).all()                  # the empty period totals 0
        again, _ = engine.period_reduce(Xd, rb, rows)
        assert torch.equal(again, got)                                               # bit-reproducible
        # powers 1..4 in one call
        got, st = engine.period_reduce(Xd, rb, rows, poly=(KELVIN, 1, 4))
        assert got.shape == (4, P, n) and int(st.item()) == 0
        for k in range(4):
            f = np.nan_to_num(O.tas_poly_values(X, k + 1), nan=0.0)
            _ok(got[k].cpu().numpy(), _psum(f, rb, rows), rtol, _psum(np.abs(f), rb, rows))
        # degree days at three thresholds: the library's own elementwise transform, summed here in fp64
        got, st = engine.period_reduce(Xd, rb, rows, X2=Hd, edd=(KELVIN, thr))
        assert got.shape == (3, P, n) and int(st.item()) == 0
        for k, e in enumerate(thr):
            f = np.nan_to_num(engine.transform_edd(Xd, Hd, KELVIN, [(1.0, e)]).cpu().numpy(), nan=0.0)
            _ok(got[k].cpu().numpy(), _psum(f, rb, rows), SUM_TOL[dtype], _psum(np.abs(f), rb, rows))
            cmin, cmax = X + dtype(KELVIN), H + dtype(KELVIN)
            o = np.nan_to_num(O.snyder_edd_values(cmin, cmax, e), nan=0.0)
            _rel_ok(got[k].cpu().numpy(), _psum(o, rb, rows), rtol, scale=0.05 * max(1, T))


def test_kernel_status_word_and_bad_lists(torch_cuda):
    """Bit 0 of the status word: an input +-inf, a power that overflows -- nothing else; row lists outside the field are
    refused (host lists in Python, device lists by the library's own check) and never read."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    X = torch.full((9, 63), 2.0, dtype=torch.float32, device="cuda")
    rb, rows = [0, 9], np.arange(9)
    assert int(engine.period_reduce(X, rb, rows)[1].item()) == 0
    X[3, 7] = float("inf")
    got, st = engine.period_reduce(X, rb, rows)
    assert int(st.item()) == 1 and torch.isinf(got[0, 0, 7]) and float(got[0, 0, 8]) == 18.0
    X[5, 7] = float("-inf")
    got, st = engine.period_reduce(X, rb, rows)
    assert int(st.item()) == 1 and torch.isnan(got[0, 0, 7])
    X[3, 7] = X[5, 7] = 1e10                                   # finite, but its 4th power is not in fp32
    assert int(engine.period_reduce(X, rb, rows, poly=(0.0, 1, 3))[1].item()) == 0
    got, st = engine.period_reduce(X, rb, rows, poly=(0.0, 1, 4))
    assert int(st.item()) == 1 and torch.isinf(got[3, 0, 7]) and torch.isfinite(got[2, 0, 7])
    assert int(engine.period_reduce(X.double(), rb, rows, poly=(0.0, 1, 4))[1].item()) == 0      # fp64 holds 1e40
    X[:] = float("nan")
    assert int(engine.period_reduce(X, rb, rows, keep_nan=True)[1].item()) == 0                   # NaN is not inf
    with pytest.raises(ValueError):
        engine.period_reduce(X, [0, 2], [0, 9])
    bad_rb = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    bad_rows = torch.tensor([0, 9], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.WaggError) as e:
        engine.period_reduce(X, bad_rb, bad_rows)
    assert e.value.code == -1 and "row" in str(e.value)
    X[:] = 1.0
    got, _ = engine.period_reduce(X, bad_rb, bad_rows, checked=True)     # vouched for, wrongly: row 9 is skipped, not read
    assert float(got[0, 0, 0]) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the public call: both routes on both plan kinds
# ---------------------------------------------------------------------------------------------------------------------
class _Case:
    """A small grid with a segment table: region 0 is a giant (half of all rows), region R - 1 has no weight at all (its
    result is NaN), popwt is <= 0 or NaN on some rows (the backup column stands in)."""

    def __init__(self, nlat, nlon, T, R, dtype, seed):
        rng = np.random.default_rng(seed)
        self.nlat, self.nlon, self.T, self.R, self.dtype = nlat, nlon, T, R, dtype
        self.lat, self.lon = np.arange(nlat) * 0.5 - 10.0, np.arange(nlon) * 0.5 + 100.0
        G = self.G = nlat * nlon
        nseg = 2 * G + 7
        cell = rng.integers(0, G, nseg)
        code = rng.integers(1, R - 1, nseg)
        code[:nseg // 2] = 0
        code[nseg // 2:nseg // 2 + R - 2] = np.arange(1, R - 1)
        code[-5:] = R - 1
        areawt, popwt = rng.uniform(0.1, 1.0, nseg), rng.uniform(-0.3, 2.0, nseg)
        popwt[rng.uniform(size=nseg) < 0.05] = np.nan
        areawt[-5:] = popwt[-5:] = 0.0
        self.cell, self.code = cell.astype(np.int32), code.astype(np.int32)
        self.w_eff = np.where(popwt > 0, popwt, areawt)
        self.df = pd.DataFrame({"lat": self.lat[cell // nlon], "lon": self.lon[cell % nlon], "areawt": areawt, "popwt": popwt, "reg": code})
        self.time = np.datetime64("2001-01-01") + np.arange(T)
        self.tas = (280 + 15 * rng.standard_normal((T, nlat, nlon))).astype(dtype)
        self.tasmax = (self.tas + rng.uniform(0, 12, self.tas.shape)).astype(dtype)
        self.rtol = RTOL32 if dtype == np.float32 else RTOL64

    def dataset(self, torch, device=True, **fields):
        from climate_toolbox_amd import minixr
        wrap = (lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()) if device else (lambda v: v)
        fields = fields or {"tas": self.tas}
        return minixr.Dataset({k: (("time", "lat", "lon"), wrap(v)) for k, v in fields.items()},
                              coords={"time": self.time, "lat": self.lat, "lon": self.lon})

    def oracle(self, f, rb, rows):
        """(period totals of the daily oracle on f, the same on |f|)"""
        from oracle import ref_numpy as O
        f2 = np.asarray(f).reshape(self.T, self.G)
        daily = O.agg_coded(f2, self.cell, self.code, self.w_eff, self.R)
        with np.errstate(invalid="ignore"):
            absd = O.agg_coded(np.abs(np.nan_to_num(f2, nan=0.0, posinf=0.0, neginf=0.0)), self.cell, self.code, self.w_eff, self.R)
        return _psum(daily, rb, rows), _psum(absd, rb, rows)


@pytest.fixture(params=["segment", "dense"])
def plan_kind(request, monkeypatch):
    """Which family serves the table: a segment-table plan, or a dense-family plan forced from the same table
    (``DensePlan.from_segments`` through the package's own family switch)."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _plans
    pkg.clear_caches()
    # (left to itself the family switch may take either for tables this small: pin it both ways)
    dense = request.param == "dense"
    monkeypatch.setattr(_plans, "_wants_dense", lambda n_ucells, G, layout, **k: dense and layout == "TG")
    yield request.param
    pkg.clear_caches()


def _spy(monkeypatch):
    """Records keep_nan of every engine.period_reduce call: False = the field was summed (reduce-first), True = the result"""
    from climate_toolbox_amd import engine
    calls, real = [], engine.period_reduce

    def wrapped(*a, **k):
        calls.append(bool(k.get("keep_nan", False)))
        return real(*a, **k)
    monkeypatch.setattr(engine, "period_reduce", wrapped)
    return calls


CASES = [(7, 9, 70, 5, np.float32), (7, 9, 9, 5, np.float64), (16, 16, 9, 40, np.float32), (16, 16, 70, 40, np.float64),
         (7, 9, 1, 5, np.float32)]


@pytest.mark.parametrize("nlat,nlon,T,R,dtype", CASES)
def test_period_totals_match_the_oracle_on_both_routes(torch_cuda, plan_kind, monkeypatch, nlat, nlon, T, R, dtype):
    """Plain, Kelvin-shifted, powers 1..4 in one call, degree days (one threshold; a three-term combination; snyder_gdd):
    every period structure, both routes, against the oracle and against each other; the plan kind that served the call is
    the one asked for."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, minixr, periods
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius, snyder_edd, snyder_gdd, tas_poly_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Case(nlat, nlon, T, R, dtype, seed=nlat + T + R)
    calls = _spy(monkeypatch)
    cmin, cmax = c.tas + dtype(KELVIN), c.tasmax + dtype(KELVIN)
    e_own = float(cmin[0, 0, 1])                                # a threshold equal to one cell's tasmin
    e_max = float(cmax[0, 0, 2])                                # ... and to one cell's tasmax

    def variables():
        """name -> (dataset holding it, the transformed daily field of the oracle)"""
        out = {"tas": (c.dataset(torch), c.tas)}
        ds = convert_kelvin_to_celsius(c.dataset(torch), "tas")
        out["tas_c"] = (minixr.Dataset({"tas_c": ds["tas"]}, coords=dict(ds.coords)), O.tas_poly_values(c.tas, 1))
        ds = c.dataset(torch, tasmin=c.tas, tasmax=c.tasmax)
        for k in ("tasmin", "tasmax"):
            ds[k].attrs["units"] = "K"
            ds = convert_kelvin_to_celsius(ds, k)
        ds["edd"] = snyder_edd(ds.tasmin, ds.tasmax, e_own)
        ds["gdd"] = snyder_gdd(ds.tasmin, ds.tasmax, 10, e_max)
        lo = ds["tasmin"]
        ds["edd3"] = minixr.LazyArray(lo._values, lo.dims, edd=(ds["tasmax"]._values, KELVIN, [(1.0, 8.0), (-0.5, e_own), (0.25, 20.0)]), name="edd3")
        out["edd"] = (ds, O.snyder_edd_values(cmin, cmax, e_own))
        out["gdd"] = (ds, O.snyder_gdd_values(cmin, cmax, 10, e_max))
        out["edd3"] = (ds, O.snyder_edd_values(cmin, cmax, 8.0) - dtype(0.5) * O.snyder_edd_values(cmin, cmax, e_own)
                       + dtype(0.25) * O.snyder_edd_values(cmin, cmax, 20.0))
        return out

    vs = variables()
    for sname, lab in _structures(T):
        labels, rb, rows = periods.period_rows(c.time, lab)
        for name, (ds, f) in vs.items():
            ref, absref = c.oracle(f, rb, rows)
            if name in ("edd", "gdd", "edd3"):
                absref = np.maximum(absref, 0.05 * max(1, T))    # (the fp32 degree-day polynomial: 2e-6 absolute per value)
            got = {}
            for route in ("reduce_first", "aggregate_first"):
                del calls[:]
                out = pkg.weighted_aggregate_grid_to_regions_periods(ds, name, "popwt", "reg", c.df, period=lab, _route=route)
                assert calls and all(k == (route == "aggregate_first") for k in calls), (route, calls)
                assert out[name].dims == ("period", "reg") and "time" not in out.coords
                np.testing.assert_array_equal(out["period"].values, labels)
                np.testing.assert_array_equal(out["reg"].values, np.arange(R))
                got[route] = out[name].values
                assert got[route].dtype == dtype and np.isnan(got[route][:, R - 1]).all()      # the region without weight
                _ok(got[route], ref, c.rtol, absref)
            _ok(got["reduce_first"], got["aggregate_first"], c.rtol, absref)
        # powers 1..4 in one pass (tas_poly_aggregate with period=): the day labels are YYYYDDD there
        for route in ("reduce_first", "aggregate_first"):
            out = tas_poly_aggregate(c.dataset(torch), [1, 2, 3, 4], "popwt", "reg", c.df, period=lab, _route=route)
            for p in (1, 2, 3, 4):
                ref, absref = c.oracle(O.tas_poly_values(c.tas, p), rb, rows)
                assert out["tas-poly-%d" % p].dims == ("period", "reg")
                _ok(out["tas-poly-%d" % p].values, ref, c.rtol, absref)
    from climate_toolbox_amd._plans import _PLAN_CACHE
    kinds = {type(p).__name__ for p in _PLAN_CACHE.values()}
    assert kinds == ({"DensePlan"} if plan_kind == "dense" else {"SparsePlan"}), kinds


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values_follow_the_daily_path(torch_cuda, plan_kind, monkeypatch, dtype):
    """NaN cells on some days count 0, a cell that is NaN every day never counts; +inf on one day and -inf on another in one
    cell give exactly the oracle's NaN / inf pattern on BOTH routes -- reduce-first must have noticed (status word) and
    redone the call aggregate-first; the same for an fp32 value whose 4th power overflows."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd.transformations import tas_poly
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Case(7, 9, 9, 5, dtype, seed=77)
    lab = np.arange(9) % 2
    labels, rb, rows = pkg.periods.period_rows(c.time, lab)
    calls = _spy(monkeypatch)
    iy, ix = divmod(int(c.cell[0]), c.nlon)                     # a cell the giant region owns with weight
    c.tas[1, 2, 3] = c.tas[4, 0, 0] = np.nan
    c.tas[:, 6, 8] = np.nan
    ds = c.dataset(torch)
    ref, absref = c.oracle(c.tas, rb, rows)
    for route in ("reduce_first", "aggregate_first"):
        del calls[:]
        _ok(pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "reg", c.df, period=lab, _route=route).tas.values,
            ref, c.rtol, absref)
        assert calls == [route == "aggregate_first"]
    c.tas[0, iy, ix], c.tas[2, iy, ix] = np.inf, -np.inf        # rows 0 and 2: the same period
    ds = c.dataset(torch)
    ref, absref = c.oracle(c.tas, rb, rows)
    assert np.isnan(ref[0, 0]) and np.isfinite(ref[1, :-1]).all()
    for route in ("reduce_first", "aggregate_first"):
        del calls[:]
        _ok(pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "reg", c.df, period=lab, _route=route).tas.values,
            ref, c.rtol, absref)
        assert calls == ([False, True] if route == "reduce_first" else [True])          # summed the field, saw inf, started over
    c.tas[0, iy, ix], c.tas[2, iy, ix] = 280.0, 1e10 if dtype == np.float32 else 290.0  # (1e10)^4 overflows fp32
    ds = tas_poly(c.dataset(torch), 4, "t4")
    f = O.tas_poly_values(c.tas, 4)
    assert np.isinf(f).any() == (dtype == np.float32)
    ref, absref = c.oracle(f, rb, rows)
    for route in ("reduce_first", "aggregate_first"):
        del calls[:]
        _ok(pkg.weighted_aggregate_grid_to_regions_periods(ds, "t4", "popwt", "reg", c.df, period=lab, _route=route).t4.values,
            ref, c.rtol, absref)
        assert calls == ([False, True] if route == "reduce_first" and dtype == np.float32 else [route == "aggregate_first"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_period_per_row_is_the_daily_call_bit_for_bit(torch_cuda, plan_kind, dtype):
    """A one-term sum through fp64 is exact: with one period per row and no transform either route returns the bits of the
    plain daily call; calling twice gives the same bits."""
    import climate_toolbox_amd as pkg
    torch = torch_cuda
    c = _Case(16, 16, 9, 40, dtype, seed=5)
    ds = c.dataset(torch)
    daily = pkg.weighted_aggregate_grid_to_regions(ds, "tas", "popwt", "reg", c.df).tas.values
    assert daily.shape == (9, 40)
    for route in ("reduce_first", "aggregate_first", None):
        out = pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "reg", c.df, period=np.arange(9), _route=route).tas.values
        np.testing.assert_array_equal(out, daily)
        out2 = pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "reg", c.df, period=np.arange(9) // 4, _route=route).tas.values
        out3 = pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", "popwt", "reg", c.df, period=np.arange(9) // 4, _route=route).tas.values
        np.testing.assert_array_equal(out2, out3)


def test_automatic_route_host_fields_other_layouts_and_device_results(torch_cuda, plan_kind, monkeypatch):
    """The automatic choice: a device-resident (time, lat, lon) field on a dense-family plan follows REDUCE_FIRST_FAMILIES,
    everything else -- a segment-table plan, a host-resident field, a (lat, lon, time) field -- aggregates first; all of
    them give the oracle's values.  results_on_device() is honoured."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import minixr, periods
    torch = torch_cuda
    c = _Case(7, 9, 70, 5, np.float32, seed=9)
    calls = _spy(monkeypatch)
    labels, rb, rows = periods.period_rows(c.time, "month")
    assert list(labels) == [200101, 200102, 200103]
    ref, absref = c.oracle(c.tas, rb, rows)
    dev = pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch), "tas", "popwt", "reg", c.df, period="month")
    family = "dense" if plan_kind == "dense" else "segment"
    assert calls == [family not in periods.REDUCE_FIRST_FAMILIES]
    _ok(dev.tas.values, ref, c.rtol, absref)
    np.testing.assert_array_equal(dev["period"].values, labels)
    del calls[:]
    host = pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch, device=False), "tas", "popwt", "reg", c.df, period="month")
    assert calls == [True] and isinstance(host.tas.data, np.ndarray)
    _ok(host.tas.values, ref, c.rtol, absref)
    _ok(host.tas.values, dev.tas.values, c.rtol, absref)
    del calls[:]
    gt = minixr.Dataset({"tas": (("lat", "lon", "time"), torch.from_numpy(np.ascontiguousarray(np.moveaxis(c.tas, 0, -1))).cuda())},
                        coords={"time": c.time, "lat": c.lat, "lon": c.lon})
    out = pkg.weighted_aggregate_grid_to_regions_periods(gt, "tas", "popwt", "reg", c.df, period="month")
    assert calls == [True] and out.tas.dims == ("reg", "period")
    _ok(out.tas.values.T, ref, c.rtol, absref)
    with pytest.raises(ValueError):
        pkg.weighted_aggregate_grid_to_regions_periods(gt, "tas", "popwt", "reg", c.df, period="month", _route="reduce_first")
    with pkg.results_on_device():
        on = pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch), "tas", "popwt", "reg", c.df, period="month")
        assert isinstance(on.tas.data, torch.Tensor) and on.tas.data.is_cuda and tuple(on.tas.data.shape) == (3, 5)
    np.testing.assert_array_equal(on.tas.values, dev.tas.values)


# ---------------------------------------------------------------------------------------------------------------------
# drop-in behaviour
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_fixture_years_and_months(ref_fixture, torch_cuda):
    """The reference's own test fixture ((lat, lon, time), ten days around a new year): dims, coords, labels, values."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import minixr
    fx, gold = ref_fixture
    time = np.datetime64("2003-12-27") + np.arange(10)
    ds = minixr.Dataset({"temperature": (["lat", "lon", "time"], fx["temp"])}, coords={"lon": fx["lon"], "lat": fx["lat"], "time": time})
    df = pd.DataFrame({"lat": fx["seg_lat"], "lon": fx["seg_lon"], "areawt": fx["areawt"], "popwt": fx["popwt"], "hierid": fx["hierid"],
                       "ISO": fx["ISO"]})
    df.index.names = ["reshape_index"]
    daily = gold["expect_popwt_ISO"]                                                  # (ISO, time)
    for period, labels, cut in (("year", [2003, 2004], [0, 5, 10]), ("month", [200312, 200401], [0, 5, 10])):
        out = pkg.weighted_aggregate_grid_to_regions_periods(ds, "temperature", "popwt", "ISO", df, period=period)
        assert out.temperature.dims == ("ISO", "period") and "time" not in out.coords and "time" not in out.dims
        assert list(out["period"].values) == labels
        np.testing.assert_array_equal(out["ISO"].values, gold["labels_ISO"])
        ref = np.stack([daily[:, a:b].sum(axis=1) for a, b in zip(cut[:-1], cut[1:])], axis=1)
        _rel_ok(out.temperature.values, ref, RTOL64)
    single = pkg.weighted_aggregate_grid_to_regions(ds, "temperature", "popwt", "ISO", df)
    assert single.temperature.dims == ("ISO", "time")                                 # the single call is what it was


def test_tas_poly_aggregate_with_a_period(torch_cuda):
    """tas_poly_aggregate(..., period="year") = tas_poly followed by the new function; period=None is today's output bit
    for bit."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import aggregations as A, minixr
    from climate_toolbox_amd.periods import period_rows
    from climate_toolbox_amd.transformations import KELVIN as K, _day_index, remove_leap_days, tas_poly, tas_poly_aggregate
    from oracle import ref_numpy as O
    c = _Case(7, 9, 70, 5, np.float32, seed=21)
    c.time = np.datetime64("2003-12-01") + np.arange(70)                               # 31 days of 2003, 39 of 2004

    def mk():
        return minixr.Dataset({"tas": (("time", "lat", "lon"), c.tas)}, coords={"time": c.time, "lat": c.lat, "lon": c.lon})

    powers = [1, 2, 3, 4]
    year = tas_poly_aggregate(mk(), powers, "popwt", "reg", c.df, period="year")
    assert list(year["period"].values) == [2003, 2004]
    _, rb, rows = period_rows(c.time, "year")
    for p in powers:
        one = pkg.weighted_aggregate_grid_to_regions_periods(tas_poly(mk(), p, "tas-poly-%d" % p), "tas-poly-%d" % p, "popwt", "reg", c.df,
                                                             period="year")
        assert one["tas-poly-%d" % p].dims == year["tas-poly-%d" % p].dims == ("period", "reg")
        ref, absref = c.oracle(O.tas_poly_values(c.tas, p), rb, rows)
        _ok(year["tas-poly-%d" % p].values, ref, c.rtol, absref)
        _ok(year["tas-poly-%d" % p].values, one["tas-poly-%d" % p].values, c.rtol, absref)
    none = tas_poly_aggregate(mk(), powers, "popwt", "reg", c.df, period=None)
    ds = remove_leap_days(mk())
    ds = minixr.Dataset({"tas": ds["tas"]}, coords={k: (minixr.DataArray(_day_index(ds), ("time",)) if k == "time" else v)
                                                  for k, v in ds.coords.items()})
    res, rdims, coords, _ = A._aggregate_core(A._reindex_spatial_data_to_regions(ds, c.df), "tas", "popwt", "reg", c.df, "areawt",
                                              powers=powers, offset=-K)
    assert rdims == ("time", "reg")
    for p, r in zip(powers, res):
        assert none["tas-poly-%d" % p].dims == ("time", "reg")
        np.testing.assert_array_equal(none["tas-poly-%d" % p].values, r)
    np.testing.assert_array_equal(none["time"].values, coords["time"])
