"""One canonical case in LABEL space, its presentations under every stored layout, and the side-field grids -- the HIP-free
half of tests/test_gpu_public_layouts.py (tests/test_public_layouts_host.py checks this module on the CPU).

The case: a field ``F[t, i, j]`` on ascending ``lat[i]`` / ``lon[j]``, a segment table given by labels, per-cell season windows
``W[i, j]`` and per-cell thresholds ``Th[k, m, i, j]``.  The expected value of every public period call is computed once, in fp64,
from these arrays: the per-cell statistic by the restatements tests/ already holds, aggregated by ``oracle.ref_numpy.agg_coded``
on ``cell = i * nlon + j``.  Nothing in an expected value knows about layouts.

``present(case, p)`` writes the same numbers under the same labels in another stored order; ``canonical(result)`` brings a result
back to ``(leading, period, reg)``.  ``side_season`` / ``side_thresholds`` hand the side fields over on a grid of their own:

  S0  the dataset's labels in the dataset's order, dims (lat, lon); thresholds from a host fp64 array; ``season_windows``
  S1  a superset -- one more latitude, one more longitude, their cells holding extremes --, latitudes DESCENDING, longitudes
      rolled (by another amount than any presentation's), dims (lon, lat); thresholds from a device tensor of the OTHER element
      type where the caller gives ``wrap``; ``get_daily_growing_season_mask``

``WRONG_JOINS`` restates, in label space, what each wrong index decision of the Python layer would compute: a wrong join hands
cell ``c`` the side value of cell ``sigma[c]`` (or of an S1 extra cell)."""
import functools
from collections import namedtuple

import numpy as np
import pandas as pd

from tests import exposure_ref as ER
from tests.cell_spell_ref import cell_spell_ref
from tests.cell_spell_rows_ref import cell_spell_rows_ref
from tests.quantile_ref import quantile_ref
from tests.rolling_ref import rolling_ref
from tests.spell_ref import in_season, spell_ref
from tests.spell_span_ref import spell_span_ref
from tests.test_gpu_parity import RTOL32, RTOL64
from tests.test_hinge_host import hinge, rcspline_terms

F32, F64 = np.float32, np.float64
RTOL = {F32: RTOL32, F64: RTOL64}
# (nlat, nlon) -> (k: the roll of the "rolled" file order, e: the longitudes east of 180 in the 0..360 file).  2k != nlon and
# 2e != nlon: neither permutation is its own inverse.  6 x 10 and 7 x 9 have rows that are no whole quads, so cells="referenced"
# falls back to whole rows there by design; 8 x 12 is the smallest grid whose rows are whole quads in BOTH orders with nlat != nlon
# -- there the packed columns are real (its rolls are multiples of 4, so the table's quads stay under 80 % of the row).
GRIDS = {(6, 10): (4, 3), (7, 9): (4, 2), (8, 12): (4, 8)}
T = 73                                                   # 22 December 2003 .. 3 March 2004: a year end and a 29 February
R = 8
OPEN = 0 | 1023 << 10
EXTRA_LON = 0.0                                          # S1's extra longitude: no grid here has it
FAR = -1.0e6                                             # S1's extra thresholds: every day is hot there

Presentation = namedtuple("Presentation", ["name", "dims", "lon", "device"])
TLL, LLT, TOA, OAT, ATO = ("time", "lat", "lon"), ("lat", "lon", "time"), ("time", "lon", "lat"), ("lon", "lat", "time"), ("lat", "time", "lon")
PRESENTATIONS = (
    Presentation("P0", TLL, "sorted", True), Presentation("P1", LLT, "sorted", True), Presentation("P2", TOA, "sorted", True),
    Presentation("P3", OAT, "sorted", True), Presentation("P4", ATO, "sorted", True), Presentation("P5", TLL, "rolled", True),
    Presentation("P6", TLL, "360", True), Presentation("P7a", TOA, "rolled", True), Presentation("P7b", OAT, "rolled", True),
    Presentation("P8-P2", TOA, "sorted", False), Presentation("P8-P5", TLL, "rolled", False), Presentation("P8-P7a", TOA, "rolled", False))
BY_NAME = {p.name: p for p in PRESENTATIONS}
SIDES = ("S0", "S1")


def pack_windows(z1, z2):
    """integer planting / harvest days (NaN: none) -> packed windows by the layout of include/wagg.h (this module's own packing)"""
    out = np.empty(len(z1), dtype=np.int32)
    for j, (p, h) in enumerate(zip(z1, z2)):
        if p != p:
            out[j] = 1 | 1 << 21
        elif h != h:
            out[j] = 1 | 1 << 20
        else:
            out[j] = int(min(p, h)) | int(max(p, h)) << 10 | (1 << 20 if h < p else 0)
    return out


def lists_of(time, period):
    """``(labels, row_begin, rows)`` of "year" / "month" on datetime64 days, restated"""
    d = np.asarray(time).astype("datetime64[D]")
    year = d.astype("datetime64[Y]").astype(np.int64) + 1970
    lab = year if period == "year" else year * 100 + d.astype("datetime64[M]").astype(np.int64) % 12 + 1
    labels = np.unique(lab)
    rows = np.concatenate([np.flatnonzero(lab == v) for v in labels])
    return labels, np.concatenate([[0], np.cumsum([(lab == v).sum() for v in labels])]).astype(np.int64), rows.astype(np.int64)


def month_day(time):
    d = np.asarray(time).astype("datetime64[D]")
    m = d.astype("datetime64[M]")
    return (m.astype(np.int64) % 12 + 1) * 100 + (d - m.astype("datetime64[D]")).astype(np.int64) + 1


class Case:
    """the canonical arrays of one grid and element type"""

    def __init__(self, nlat, nlon, dtype):
        self.roll, self.east = GRIDS[(nlat, nlon)]
        rng = np.random.default_rng(1000 * nlat + nlon)
        self.nlat, self.nlon, self.G, self.T, self.R, self.dtype, self.rtol = nlat, nlon, nlat * nlon, T, R, dtype, RTOL[dtype]
        self.lat = -10.0 + 0.5 * np.arange(nlat)
        self.lon360 = 180.0 - 0.5 * self.east + 0.5 * np.arange(nlon)                 # the 0..360 file's labels, ascending
        self.lon = np.sort((self.lon360 + 180.0) % 360.0 - 180.0)                      # -180 .. , .. 179.5: the labels
        self.time = np.datetime64("2003-12-22") + np.arange(T)
        self.doy = ((self.time - self.time.astype("datetime64[Y]").astype("datetime64[D]")).astype(np.int64) + 1).astype(np.int32)
        assert self.doy[9] == 365 and self.doy[10] == 1 and month_day(self.time)[69] == 229
        G = self.G
        # the field: an AR(1) series per cell about 281 K, so that spells of several days exist; one NaN
        z = rng.standard_normal((T, G))
        for t in range(1, T):
            z[t] = 0.75 * z[t - 1] + 0.66 * z[t]
        tas = (281.0 + 7.0 * z + rng.uniform(-3, 3, (1, G))).astype(dtype)
        tas[5, nlon + 2] = np.nan
        self.tas = tas.reshape(T, nlat, nlon)
        self.tasmax = (tas + rng.uniform(0.5, 12.0, tas.shape).astype(dtype)).astype(dtype).reshape(T, nlat, nlon)
        # the table: on 8 x 12 the cells of three 4 x 4 blocks (half the quads in either order); elsewhere 60 % of the cells
        if (nlat, nlon) == (8, 12):
            blocks = [(0, 0), (1, 1), (0, 2)]
            cells = np.array([(4 * bi + a) * nlon + 4 * bj + b for bi, bj in blocks for a in range(4) for b in range(4)])
            cells = cells[rng.uniform(size=len(cells)) < 0.85]
        else:
            cells = np.sort(rng.choice(G, size=int(0.6 * G), replace=False))
        code = rng.integers(0, R - 1, len(cells))
        code[:R - 1] = np.arange(R - 1)
        cell = np.concatenate([cells, [cells[5], cells[9], cells[-1]]])               # a cell in two regions, a row twice
        code = np.concatenate([code, [(code[5] + 1) % (R - 1), code[9], R - 1]])
        nseg = len(cell)
        areawt, popwt = rng.uniform(0.1, 1.0, nseg), rng.uniform(-0.3, 2.0, nseg)
        popwt[rng.uniform(size=nseg) < 0.05] = np.nan
        areawt[-1] = popwt[-1] = 0.0                                                  # region R - 1 has no weight: NaN
        self.cell, self.code = cell.astype(np.int32), code.astype(np.int32)
        self.w_eff = np.where(popwt > 0, popwt, areawt)
        self.df = pd.DataFrame({"lat": self.lat[cell // nlon], "lon": self.lon[cell % nlon], "areawt": areawt, "popwt": popwt, "reg": code})
        # season windows: an interval, one that wraps the year end, no planting day (null), no harvest day -- no symmetry
        kind = rng.choice(4, size=G, p=[0.5, 0.36, 0.08, 0.06])
        z1 = rng.integers(1, 40, G).astype(np.float64)
        z2 = z1 + rng.integers(3, 30, G)
        wrap = kind == 1
        z1[wrap], z2[wrap] = rng.integers(352, 366, wrap.sum()), rng.integers(3, 35, wrap.sum())
        z1[kind == 2] = np.nan
        z2[kind == 3] = np.nan
        self.z1, self.z2 = z1.reshape(nlat, nlon), z2.reshape(nlat, nlon)
        self.W = pack_windows(z1, z2)
        # thresholds near the field's median, fp32-representable (either element type holds them exactly), two levels
        self.levels = np.array([0.5, 0.9])
        self.planes = {None: np.array([0]), "month": np.array([1, 2, 3, 12]), "calendar_day": np.unique(month_day(self.time))}
        self.Th = {k: (281.0 + 5.0 * rng.standard_normal((2, len(lab), nlat, nlon)) + np.array([0.0, 4.0])[:, None, None, None])
                   .astype(F32).astype(F64) for k, lab in self.planes.items()}

    # -- stored order ------------------------------------------------------------------------------------------------
    def lon_order(self, how):
        """label index of every buffer column of a file written "sorted", "rolled" or "360" """
        j = np.arange(self.nlon)
        return j if how == "sorted" else np.roll(j, self.roll if how == "rolled" else self.east)

    def stored_cells(self, p):
        """the canonical cell ``i * nlon + j`` at every position of presentation ``p``'s flattened (lat, lon) / (lon, lat) axes"""
        col = self.lon_order(p.lon)
        grid = np.arange(self.nlat)[:, None] * self.nlon + col[None, :]
        return (grid if p.dims.index("lat") < p.dims.index("lon") else grid.T).reshape(-1)

    def flat(self, f):
        return np.asarray(f).reshape(self.T, self.G)

    def agg(self, cells):
        """(K, P, G) per-cell values -> (K, P, R) by the fp64 oracle"""
        from oracle import ref_numpy as O
        return np.stack([O.agg_coded(c, self.cell, self.code, self.w_eff, self.R) for c in cells])

    def expected(self, cells):
        """``(want, bound)``: the label-space reference and the project's bound, RTOL * the oracle on |per-cell values|"""
        return self.agg(cells), self.rtol * self.agg(np.abs(np.nan_to_num(cells, nan=0.0)))


@functools.lru_cache(maxsize=None)
def case(nlat, nlon, dtype):
    return Case(nlat, nlon, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# presentations
# ---------------------------------------------------------------------------------------------------------------------
def present(c, p, wrap=None, fields=None):
    """the case as a minixr Dataset in presentation ``p``: variables tas / tasmin (= tas) / tasmax in Kelvin.  ``wrap``: host
    array -> device tensor, used where ``p.device``; None leaves every buffer on the host."""
    from climate_toolbox_amd import minixr, standardize_climate_data
    col = c.lon_order(p.lon)
    lon = c.lon[col] % 360.0 if p.lon == "360" else c.lon[col]
    order = [TLL.index(d) for d in p.dims]
    fields = fields or {"tas": c.tas, "tasmin": c.tas, "tasmax": c.tasmax}

    def buf(f):
        a = np.ascontiguousarray(np.transpose(f[:, :, col], order))
        return wrap(a) if p.device and wrap is not None else a

    ds = minixr.Dataset({k: (p.dims, buf(f)) for k, f in fields.items()}, coords={"time": c.time, "lat": c.lat, "lon": lon})
    if p.lon != "sorted":
        ds = standardize_climate_data(ds)
        assert all(getattr(ds[k], "_lon_perm", None) is not None for k in fields), "the presentation must leave a lazy permutation"
        perm = np.asarray(ds["tas"]._lon_perm)
        assert not np.array_equal(perm[perm], np.arange(c.nlon)), "the permutation must not be its own inverse"
    assert list(ds.coords["lon"].values) == list(c.lon)
    return ds


def canonical(var, lead=None, agglev="reg"):
    """a result variable's values as ``(lead, period, reg)`` (``lead`` None: ``(period, reg)``)"""
    want = ((lead,) if lead else ()) + ("period", agglev)
    assert sorted(var.dims) == sorted(want), (var.dims, want)
    return np.transpose(np.asarray(var.values), [var.dims.index(d) for d in want])


def result_dims(p, lead=None, agglev="reg"):
    """what ``_result_dims`` gives for ``p.dims``, restated: the region takes the slot of the first of lat / lon, the second goes,
    ``time`` becomes ``period``; a leading dim stands in front"""
    ia, io = p.dims.index("lat"), p.dims.index("lon")
    out = tuple(agglev if i == min(ia, io) else ("period" if d == "time" else d) for i, d in enumerate(p.dims) if i != max(ia, io))
    return ((lead,) if lead else ()) + out


# ---------------------------------------------------------------------------------------------------------------------
# side-field grids
# ---------------------------------------------------------------------------------------------------------------------
def side_grid(c, side):
    """``(lat, lon, ilat, ilon)``: the side grid's labels, and where the case's labels sit in them"""
    if side == "S0":
        return c.lat, c.lon, np.arange(c.nlat), np.arange(c.nlon)
    lat = np.concatenate([c.lat, [c.lat[-1] + 0.5]])[::-1].copy()
    lon = np.roll(np.concatenate([c.lon, [EXTRA_LON]]), c.roll + 1)
    assert EXTRA_LON not in c.lon
    return lat, lon, np.array([int(np.flatnonzero(lat == v)[0]) for v in c.lat]), np.array([int(np.flatnonzero(lon == v)[0]) for v in c.lon])


def on_side(c, a, side, fill):
    """``a`` (..., nlat, nlon) on the side grid, (..., lat, lon) for S0 and (..., lon, lat) for S1, ``fill`` in the extra cells"""
    lat, lon, ilat, ilon = side_grid(c, side)
    out = np.full(a.shape[:-2] + (len(lat), len(lon)), fill, dtype=a.dtype)
    out[..., ilat[:, None], ilon[None, :]] = a
    return out if side == "S0" else np.ascontiguousarray(np.swapaxes(out, -1, -2))


def growing_days(c, side, drop_lon=None):
    """the growing-days Dataset on the side grid (its longitudes are the labels + 180); S1's extra cells are open all year.
    ``drop_lon``: a longitude label left out"""
    from climate_toolbox_amd import minixr
    lat, lon, _, _ = side_grid(c, side)
    z = np.stack([on_side(c, c.z1, side, 0.0), on_side(c, c.z2, side, 1023.0)])
    dims = ("z", "latitude", "longitude") if side == "S0" else ("z", "longitude", "latitude")
    if drop_lon is not None:
        keep = lon != drop_lon
        z, lon = np.compress(keep, z, axis=dims.index("longitude")), lon[keep]
    return minixr.Dataset({"variable": (dims, z)}, coords={"z": np.array([1, 2]), "latitude": lat, "longitude": lon + 180.0})


def side_season(c, side, drop_lon=None):
    """``season=`` on the side grid: S0 through ``season_windows``, S1 through ``get_daily_growing_season_mask``"""
    import climate_toolbox_amd as pkg
    gd = growing_days(c, side, drop_lon)
    return pkg.season_windows(gd) if side == "S0" else pkg.get_daily_growing_season_mask(None, None, c.time[:3], gd)


def side_thresholds(c, kind, side, wrap=None, drop_lon=None):
    """the thresholds of plane kind ``kind`` (None / "month" / "calendar_day") on the side grid: S0 a host fp64 array, S1 -- where
    ``wrap`` is given -- a device tensor of the element type the field does NOT have"""
    from climate_toolbox_amd.relative import CellThresholds
    lat, lon, _, _ = side_grid(c, side)
    v = on_side(c, c.Th[kind], side, FAR)
    dims = ("lat", "lon") if side == "S0" else ("lon", "lat")
    if drop_lon is not None:
        keep = lon != drop_lon
        v, lon = np.compress(keep, v, axis=2 + dims.index("lon")), lon[keep]
    if side == "S1" and wrap is not None:
        v = wrap(np.ascontiguousarray(v.astype(F64 if c.dtype == F32 else F32)))
    return CellThresholds.from_array(v, lat, lon, dims=dims, labels=c.planes[kind], levels=c.levels)


def canonical_thresholds(c, th):
    """a CellThresholds' values re-indexed to ``(K, M, lat, lon)`` of the case through its own ``lat`` / ``lon`` / ``dims``"""
    v = th.values
    v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    grid = (len(th.lat), len(th.lon)) if th.dims == ("lat", "lon") else (len(th.lon), len(th.lat))
    v = v.reshape(v.shape[:2] + grid)
    v = v if th.dims == ("lat", "lon") else np.swapaxes(v, 2, 3)
    ilat = np.array([int(np.flatnonzero(th.lat == x)[0]) for x in c.lat])
    ilon = np.array([int(np.flatnonzero(th.lon == x)[0]) for x in c.lon])
    return v[:, :, ilat[:, None], ilon[None, :]]


# ---------------------------------------------------------------------------------------------------------------------
# the calls: how each is made, and its per-cell statistic in label space
# ---------------------------------------------------------------------------------------------------------------------
LADDER = [272.0, 281.0, 286.0]
EDGES = [-np.inf, 274.0, 281.0, 288.0, np.inf]
KNOTS = [276.0, 286.0]
SPLINE = [268.0, 277.0, 285.0, 294.0]
SPELL = [279.0, 284.0]
ROLL = [1, 5]
Q = [0.1, 0.5, 0.9]
ARGS = ("popwt", "reg")


def mask_of(doy, W):
    """(T, G) bool: the cell is in season on the day"""
    return np.stack([np.asarray(in_season(int(d), W), dtype=bool) for d in doy])


def _sums(c, daily, W, period="month", time=None, doy=None):
    """(K, T, G) daily values -> (K, P, G) in-season period sums, NaN counting 0"""
    time = c.time if time is None else time
    _, rb, rows = lists_of(time, period)
    return ER.period_sum(np.nan_to_num(np.asarray(daily, dtype=F64), nan=0.0), rb, rows, mask_of(c.doy if doy is None else doy, W))


def _ref_plain(c, W, Th):
    return _sums(c, c.flat(c.tas)[None], W)


def _ref_poly(c, W, Th):
    from oracle import ref_numpy as O
    keep = month_day(c.time) != 229                                    # tas_poly drops 29 February and numbers the days 1..
    X = c.flat(c.tas)[keep]
    return _sums(c, np.stack([O.tas_poly_values(X, p) for p in (1, 2, 3)]), W, "year", c.time[keep], np.arange(1, keep.sum() + 1))


def _ref_edd(c, W, Th):
    from oracle import ref_numpy as O
    return _sums(c, np.stack([O.snyder_edd_values(c.flat(c.tas), c.flat(c.tasmax), e) for e in LADDER]), W)


def _ref_exposure(c, W, Th):
    _, rb, rows = lists_of(c.time, "month")
    return ER.exposure_bins(c.flat(c.tas), c.flat(c.tasmax), 0.0, EDGES, rb, rows, mask_of(c.doy, W))


def _ref_bins(c, W, Th):
    x = c.flat(c.tas).astype(F64)
    with np.errstate(invalid="ignore"):
        return _sums(c, np.stack([(x >= EDGES[k]) & (x < EDGES[k + 1]) for k in range(len(EDGES) - 1)]).astype(F64), W)


def _ref_hinge(c, W, Th):
    return _sums(c, np.stack([hinge(c.flat(c.tas), k, 2, "above") for k in KNOTS]), W)


def _ref_spline(c, W, Th):
    return _sums(c, rcspline_terms(c.flat(c.tas), SPLINE), W)


def _by_lists(ref, **kw):
    def run(c, W, Th):
        _, rb, rows = lists_of(c.time, "month")
        return np.asarray(ref(c.flat(c.tas), rb, rows, 0.0, doy=c.doy, windows=W, **kw), dtype=F64)
    return run


def _ref_relative(kind, stat, L):
    def run(c, W, Th):
        labels, rb, rows = lists_of(c.time, "month")
        thr = Th[kind].reshape(2, -1, c.G).astype(c.dtype)
        if kind == "calendar_day":
            pmap = np.searchsorted(c.planes[kind], month_day(c.time))
            return np.asarray(cell_spell_rows_ref(c.flat(c.tas), rb, rows, 0.0, thr, pmap, L, stat, "above", c.doy, W), dtype=F64)
        pmap = None if kind is None else np.searchsorted(c.planes[kind], labels % 100)
        return np.asarray(cell_spell_ref(c.flat(c.tas), rb, rows, 0.0, thr, pmap, L, stat, "above", c.doy, W), dtype=F64)
    return run


def _t(name):
    import climate_toolbox_amd.transformations as tr
    return getattr(tr, name)


def _call_plain(ds, c, season, th, cells):
    import climate_toolbox_amd as pkg
    return pkg.weighted_aggregate_grid_to_regions_periods(ds, "tas", *ARGS, c.df, period="month", season=season, cells=cells)["tas"], None


def _call_poly(ds, c, season, th, cells):
    from climate_toolbox_amd import minixr
    out = _t("tas_poly_aggregate")(ds, [1, 2, 3], *ARGS, c.df, period="year", season=season, cells=cells)
    v = [out["tas-poly-%d" % p] for p in (1, 2, 3)]
    assert all(a.dims == v[0].dims for a in v)
    return minixr.DataArray(np.stack([np.asarray(a.values) for a in v]), ("power",) + tuple(v[0].dims)), None


def _simple(fn, var, lead, *params, **kw):
    def run(ds, c, season, th, cells):
        out = _t(fn)(ds, *params, *ARGS, c.df, period="month", season=season, cells=cells, **kw)
        return out[var], np.asarray(out[lead].values)
    return run


def _call_relative(kind, stat, L):
    def run(ds, c, season, th, cells):
        out = _t("tas_relative_spell_aggregate")(ds, th, *ARGS, c.df, period="month", planes=kind, stat=stat, min_length=L, season=season,
                                                 cells=cells)
        return out["tas-relative-spell"], np.asarray(out["threshold"].values)
    return run


Call = namedtuple("Call", ["name", "lead", "coord", "run", "ref", "thresholds"])
CALLS = (
    Call("periods", None, None, _call_plain, _ref_plain, False),
    Call("poly", "power", None, _call_poly, _ref_poly, False),
    Call("edd_ladder", "refTemp", LADDER, _simple("snyder_edd_aggregate", "edd", "refTemp", LADDER), _ref_edd, False),
    Call("exposure", "bin", EDGES[:-1], _simple("snyder_exposure_aggregate", "exposure", "bin", EDGES), _ref_exposure, False),
    Call("bins", "bin", EDGES[:-1], _simple("tas_bins_aggregate", "tas-bins", "bin", EDGES), _ref_bins, False),
    Call("hinge", "knot", KNOTS, _simple("tas_hinge_aggregate", "tas-hinge", "knot", KNOTS, power=2), _ref_hinge, False),
    Call("rcspline", "term", SPLINE[:-2], _simple("tas_rcspline_aggregate", "tas-rcspline", "term", SPLINE), _ref_spline, False),
    Call("spell_period", "threshold", SPELL, _simple("tas_spell_aggregate", "tas-spell", "threshold", SPELL, min_length=2, stat="days"),
         _by_lists(spell_ref, thresholds=SPELL, min_length=2, stat="days", side="above"), False),
    Call("spell_record", "threshold", SPELL, _simple("tas_spell_aggregate", "tas-spell", "threshold", SPELL, stat="longest", span="record"),
         _by_lists(spell_span_ref, thresholds=SPELL, min_length=1, stat="longest", side="above"), False),
    Call("relative_one_days", "threshold", [0.5, 0.9], _call_relative(None, "days", 2), _ref_relative(None, "days", 2), None),
    Call("relative_month_longest", "threshold", [0.5, 0.9], _call_relative("month", "longest", 3), _ref_relative("month", "longest", 1), "month"),
    Call("relative_day_excess", "threshold", [0.5, 0.9], _call_relative("calendar_day", "excess", 3),
         _ref_relative("calendar_day", "excess", 1), "calendar_day"),
    Call("rolling", "window", ROLL, _simple("tas_rolling_aggregate", "tas-rolling", "window", ROLL),
         _by_lists(rolling_ref, lengths=ROLL, stat="max", of="mean"), False),
    Call("quantile", "quantile", Q, _simple("tas_quantile_aggregate", "tas-quantile", "quantile", Q), _by_lists(quantile_ref, q=Q, method="linear"), False),
)
CALL = {k.name: k for k in CALLS}


@functools.lru_cache(maxsize=None)
def reference(nlat, nlon, dtype, name):
    """``(want, bound, cells)`` of call ``name`` on the canonical case: the per-cell statistic in label space, aggregated"""
    c = case(nlat, nlon, dtype)
    cells = CALL[name].ref(c, c.W, c.Th)
    return c.expected(cells) + (cells,)


# ---------------------------------------------------------------------------------------------------------------------
# wrong joins, in label space
# ---------------------------------------------------------------------------------------------------------------------
def packed_cells_model(c, p):
    """a model of the packed columns of ``cells="referenced"``: the cells of the 4-cell quads of presentation ``p``'s stored row
    that hold a referenced cell, as STORED positions in ascending order; None where the call falls back to whole rows (rows
    that are no whole quads, more than 80 % of the row).  (The plan may add a quad per chunk; the GPU test reads the real map.)"""
    row_len = c.nlon if p.dims.index("lat") < p.dims.index("lon") else c.nlat
    if row_len % 4 != 0:
        return None
    pos_of = np.empty(c.G, dtype=np.int64)
    pos_of[c.stored_cells(p)] = np.arange(c.G)
    quads = np.unique(pos_of[c.cell] // 4)
    pos = (4 * quads[:, None] + np.arange(4)[None, :]).reshape(-1)
    return None if 5 * len(pos) > 4 * c.G else pos


def wrong_sources(c, p, side):
    """``{name: src}``: for each wrong join that differs from the right one under (``p``, ``side``), the side-grid cell each
    canonical cell would read -- ``src`` (nlat, nlon, 2) of (row, column) indices into the side grid's (lat, lon) planes"""
    lat_s, lon_s, ilat, ilon = side_grid(c, side)
    col = c.lon_order(p.lon)                      # buffer column -> label
    perm = np.argsort(col)                        # label -> buffer column: the dataset's _lon_perm
    lat_first = p.dims.index("lat") < p.dims.index("lon")
    nlat, nlon = c.nlat, c.nlon

    def read(stored_of_label_plane):
        """stored (flattened buffer order) side cells -> what every canonical cell gets"""
        out = np.empty((c.G, 2), dtype=np.int64)
        out[c.stored_cells(p)] = stored_of_label_plane
        return out.reshape(nlat, nlon, 2)

    def stored(jl, jo, scatter, transpose):
        """the product's steps with the given choices: join (rows jl, columns jo), scatter into buffer columns, lay out"""
        win = np.stack(np.meshgrid(jl, jo, indexing="ij"), axis=-1)               # (nlat, nlon, 2) in label order
        st = np.empty_like(win)
        st[:, scatter] = win
        return (np.transpose(st, (1, 0, 2)) if transpose else st).reshape(-1, 2)

    right = stored(ilat, ilon, perm, not lat_first)
    out = {}
    if p.lon != "sorted":
        out["identity for the permutation"] = stored(ilat, ilon, np.arange(nlon), not lat_first)
        out["the inverse permutation"] = stored(ilat, ilon, col, not lat_first)
    out["a transposed grid"] = stored(ilat, ilon, perm, lat_first)
    if side == "S1":
        out["descending latitudes read as ascending"] = stored(len(lat_s) - 1 - ilat, ilon, perm, not lat_first)
    pos = packed_cells_model(c, p)
    if pos is not None:
        gather = right.copy()
        gather[pos] = right[:len(pos)]                                            # column k of the packed row reads stored cell k
        out["the packed-column gather omitted"] = gather
    assert np.array_equal(read(right).reshape(-1, 2), np.stack(np.meshgrid(ilat, ilon, indexing="ij"), axis=-1).reshape(-1, 2))
    return {k: read(v) for k, v in out.items() if not np.array_equal(v, right)}


def side_planes(c, side):
    """the side fields on the side grid as (lat, lon) planes: ``(W2 (nlat_s, nlon_s) packed windows, {kind: Th (K, M, nlat_s, nlon_s)})``"""
    W2 = on_side(c, c.W.reshape(c.nlat, c.nlon), "S0" if side == "S0" else "S1", np.int32(OPEN))
    th = {k: on_side(c, v, side, FAR) for k, v in c.Th.items()}
    if side == "S1":
        W2, th = np.swapaxes(W2, -1, -2), {k: np.swapaxes(v, -1, -2) for k, v in th.items()}
    return W2, th
