"""Packed rows on the GPU (run with -m gpu): engine.pack_rows / SparsePlan.compact_cells / SparsePlan.apply(compact=True) and
``cells="referenced"`` of the period calls -- the field cut down to the 16-byte quads the segment table references before it is
summed over time and contracted.

Bit-for-bit checks compare integer views (NaN payloads and signed zeros count).  End to end the oracles and tolerances are those
of tests/test_gpu_seasons.py and tests/test_gpu_edd_ladder.py (the project's 1e-4 fp32 / 1e-6 fp64 relative to the oracle on |f|);
against ``cells="all"`` only the largest relative difference is PRINTED: it comes from the split of the fp64 partial sums (n
differs), and no bound for it has been derived.

Shapes: grids 16 x 32 and 12 x 36 (rows of whole quads; the second is not a whole number of 32-cell strips), T = 40, a table of
about 30 regions on about a third of the cells that holds the first and the last quad of the grid, a quad whose only referenced
cell is the last cell of a grid row, a run of four adjacent quads, a cell shared by two regions and a duplicated row."""
import numpy as np
import pandas as pd
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64
from tests.test_gpu_periods import _Case, _ok, _psum
from tests.test_gpu_seasons import KELVIN, _mask_TG, _mixed_cells, _oracle, _pack, _seasons_for

pytestmark = pytest.mark.gpu

GRIDS = [(16, 32), (12, 36)]
T = 40
THR9 = [-40.0, 60.0, 1.5, 7.25, 0.0, 8.0, 10.5, 19.0, 30.0]            # below, inside and above the data; one group of 8 plus one


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


@pytest.fixture()
def segment_plans(monkeypatch):
    """the package's family switch pinned to segment-table plans (tables this small may go either way)"""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _plans
    pkg.clear_caches()
    monkeypatch.setattr(_plans, "_wants_dense", lambda n_ucells, G, layout, **k: False)
    yield
    pkg.clear_caches()


def _bits(a):
    """host integer view of a tensor or array"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


class _Sparse(_Case):
    """tests/test_gpu_periods.py's case with the table this module's docstring describes; ``ref_quads``: the quads that hold a
    referenced cell, ``ocean``: cells of quads no row reads"""

    def __init__(self, nlat, nlon, dtype, seed, R=30):
        rng = np.random.default_rng(seed)
        self.nlat, self.nlon, self.T, self.R, self.dtype = nlat, nlon, T, R, dtype
        self.lat, self.lon = np.arange(nlat) * 0.5 - 10.0, np.arange(nlon) * 0.5 + 100.0
        G = self.G = nlat * nlon
        nq = G // 4
        quads = set(rng.choice(nq, size=int(0.3 * nq), replace=False).tolist())
        lone = (3 * nlon + nlon - 4) // 4                                 # the last quad of grid row 3: only its last cell
        run = [(6 * nlon) // 4 + 1 + k for k in range(4)]                  # four adjacent quads
        quads |= {0, nq - 1, *run}
        quads -= {lone, lone - 1}
        cells = np.array(sorted(4 * q + k for q in quads for k in range(4)))
        cells = cells[rng.uniform(size=len(cells)) < 0.9]
        cells = np.unique(np.concatenate([cells, [0, 3, G - 4, G - 1, 3 * nlon + nlon - 1], [4 * q for q in run]]))
        code = rng.integers(1, R - 1, len(cells))
        code[:len(cells) // 3] = 0
        code[len(cells) // 3:len(cells) // 3 + R - 2] = np.arange(1, R - 1)
        shared = cells[5]                                                 # one cell in two regions, one row twice
        cell = np.concatenate([cells, [shared, cells[9], G - 1]])
        code = np.concatenate([code, [(code[5] + 1) % (R - 1), code[9], R - 1]])
        nseg = len(cell)
        areawt, popwt = rng.uniform(0.1, 1.0, nseg), rng.uniform(-0.3, 2.0, nseg)
        popwt[rng.uniform(size=nseg) < 0.05] = np.nan
        areawt[-1] = popwt[-1] = 0.0                                      # region R - 1 has no weight: NaN
        self.cell, self.code = cell.astype(np.int32), code.astype(np.int32)
        self.w_eff = np.where(popwt > 0, popwt, areawt)
        self.df = pd.DataFrame({"lat": self.lat[cell // nlon], "lon": self.lon[cell % nlon], "areawt": areawt, "popwt": popwt, "reg": code})
        self.time = np.datetime64("2001-01-01") + np.arange(T)
        self.ref_quads = np.unique(cell // 4)
        assert lone in self.ref_quads and len(np.unique(cell)) < 0.4 * G
        ocean_q = np.setdiff1d(np.arange(nq), self.ref_quads)
        self.ocean = (4 * ocean_q[:, None] + np.arange(4)[None, :]).reshape(-1)
        tas = (280 + 15 * rng.standard_normal((T, G))).astype(dtype)
        tasmax = (tas + rng.uniform(0, 12, tas.shape)).astype(dtype)
        tasmax[:, cells[7]] = tas[:, cells[7]]                            # tasmin = tasmax somewhere
        tas[2, cells[3]] = np.nan                                         # NaN in a referenced cell
        tasmax[5, cells[11]] = np.nan
        self.tas, self.tasmax = tas.reshape(T, nlat, nlon), tasmax.reshape(T, nlat, nlon)
        self.rtol = RTOL32 if dtype == np.float32 else RTOL64

    def poisoned(self, f, packed=()):
        """``f`` with NaN, +inf and -inf in cells of quads no row reads (and that are not among the cells ``packed``)"""
        g = f.reshape(T, self.G).copy()
        oc = np.setdiff1d(self.ocean, np.asarray(packed, dtype=np.int64))
        assert len(oc) > self.G // 4
        g[:, oc[0::3]], g[1::2, oc[1::3]], g[0::2, oc[2::3]] = np.nan, np.inf, -np.inf
        return g.reshape(f.shape)

    def plan(self, flags=0):
        from climate_toolbox_amd.engine import SparsePlan
        return SparsePlan(self.cell, self.code, self.w_eff, self.G, self.R, row_len=self.nlon, flags=flags)


def _lists(torch):
    """CSR row lists over T = 40 rows: three uneven periods, an empty one, a dropped row (row 7), one list not in time order"""
    a, b, c = np.arange(0, 5), np.concatenate([np.arange(5, 7), np.arange(8, 18)]), np.arange(18, T)
    c = c[np.random.default_rng(3).permutation(len(c))]
    rows = np.concatenate([a, b, c])
    rb = np.array([0, len(a), len(a), len(a) + len(b), len(rows)])
    return rb, rows


def _strided(torch, host, pad):
    buf = torch.zeros((host.shape[0], host.shape[1] + pad), dtype=torch.float32 if host.dtype == np.float32 else torch.float64, device="cuda")
    buf[:, :host.shape[1]] = torch.from_numpy(host).cuda()
    return buf[:, :host.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------
# the compact row and the pack kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nlat,nlon", GRIDS)
def test_pack_rows_on_the_device_is_the_column_gather(torch_cuda, nlat, nlon, dtype):
    """compact_cells: whole aligned quads in ascending grid order, every referenced quad among them, well under 80 % of the row;
    pack_rows(X) == X[:, compact_cells] bit for bit -- one field and two, contiguous, pitched by whole quads (16-byte pieces),
    pitched by 3 elements and offset by one element (the element-wise kernel)."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    c = _Sparse(nlat, nlon, dtype, seed=nlat)
    plan = c.plan()
    cells = plan.compact_cells(dtype)
    assert cells is not None and cells.dtype == np.int32 and len(cells) % 4 == 0 and plan.compact_cells(dtype) is cells
    q = cells.reshape(-1, 4)
    assert (q[:, 0] % 4 == 0).all() and (q == q[:, :1] + np.arange(4)).all() and (np.diff(q[:, 0]) > 0).all()
    assert np.isin(4 * c.ref_quads, q[:, 0]).all() and 5 * len(cells) <= 4 * c.G
    Gq = len(cells)
    X = c.poisoned(c.tas).reshape(T, c.G)
    H = c.poisoned(c.tasmax).reshape(T, c.G)
    before = dict(engine.PACK_STATS)
    for name, Xd, Hd in (("contiguous", torch.from_numpy(X).cuda(), torch.from_numpy(H).cuda()),
                         ("pitched by two quads", _strided(torch, X, 8), _strided(torch, H, 8)),
                         ("pitched by 3 elements", _strided(torch, X, 3), _strided(torch, H, 3))):
        one = engine.pack_rows(plan, Xd)
        assert tuple(one.shape) == (T, Gq) and one.dtype == Xd.dtype
        np.testing.assert_array_equal(_bits(one), _bits(X[:, cells]), err_msg=name)
        two = engine.pack_rows(plan, Xd, Hd)
        assert tuple(two.shape) == (T, 2 * Gq)
        np.testing.assert_array_equal(_bits(two[:, :Gq]), _bits(X[:, cells]), err_msg=name)
        np.testing.assert_array_equal(_bits(two[:, Gq:]), _bits(H[:, cells]), err_msg=name)
    flat = torch.zeros(T * c.G + 1, dtype=one.dtype, device="cuda")
    flat[1:] = torch.from_numpy(X.reshape(-1)).cuda()
    off = flat[1:].view(T, c.G)
    assert off.data_ptr() % 16 != 0
    np.testing.assert_array_equal(_bits(engine.pack_rows(plan, off)), _bits(X[:, cells]))
    np.testing.assert_array_equal(_bits(engine.pack_rows(plan, off[:1])), _bits(X[:1, cells]))       # a single row
    assert engine.PACK_STATS["device"] == before["device"] + 8 and engine.PACK_STATS["host"] == before["host"]
    with pytest.raises(ValueError):
        engine.pack_rows(plan, off[:, :c.G - 4])
    with pytest.raises(ValueError):
        engine.pack_rows(plan, torch.from_numpy(X).cuda(), _strided(torch, H, 4))                     # two row strides


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nlat,nlon", GRIDS)
def test_reductions_of_packed_rows_equal_the_columns_of_the_full_field(torch_cuda, nlat, nlon, dtype):
    """period_reduce, season_reduce and edd_ladder_reduce (nine thresholds) on the packed matrix, windows gathered through
    compact_cells, against the same call on the full field taken at compact_cells -- plane by plane, bit for bit, with no
    workspace on either side (one part per list: the split cannot depend on n).  Windows: all-year, null, empty, a single day,
    an interval and one that wraps the year end; NaN in season counts 0; the status words agree."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    c = _Sparse(nlat, nlon, dtype, seed=nlat + 1)
    plan = c.plan()
    cells = plan.compact_cells(dtype)
    Gq = len(cells)
    X, H = c.tas.reshape(T, c.G), c.tasmax.reshape(T, c.G)                        # (finite outside the NaN the case plants)
    Xd, Hd = torch.from_numpy(X).cuda(), torch.from_numpy(H).cuda()
    packed = engine.pack_rows(plan, Xd, Hd)
    Xp, Hp = packed[:, :Gq], packed[:, Gq:]
    rb, rows = _lists(torch)
    doy = np.concatenate([np.arange(346, 366), np.arange(1, T - 19)])            # across a year end
    z1, z2 = _mixed_cells(c.G, doy)
    win = _pack(z1, z2)
    idx = torch.from_numpy(cells.astype(np.int64)).cuda()
    thr3 = [float(X[0, cells[1]] + dtype(KELVIN)), 12.5, 60.0]
    kw = dict(workspace=False)
    calls = [("period", lambda A, B, w: engine.period_reduce(A, rb, rows, **kw)),
             ("period poly", lambda A, B, w: engine.period_reduce(A, rb, rows, poly=(KELVIN, 1, 4), **kw)),
             ("period edd", lambda A, B, w: engine.period_reduce(A, rb, rows, X2=B, edd=(KELVIN, thr3), **kw)),
             ("season", lambda A, B, w: engine.season_reduce(A, rb, rows, doy, w, **kw)),
             ("season poly", lambda A, B, w: engine.season_reduce(A, rb, rows, doy, w, poly=(KELVIN, 1, 4), **kw)),
             ("season edd", lambda A, B, w: engine.season_reduce(A, rb, rows, doy, w, X2=B, edd=(KELVIN, thr3), **kw)),
             ("ladder", lambda A, B, w: engine.edd_ladder_reduce(A, B, rb, rows, KELVIN, THR9, **kw)),
             ("ladder season", lambda A, B, w: engine.edd_ladder_reduce(A, B, rb, rows, KELVIN, THR9, doy=doy, windows=w, **kw))]
    for name, call in calls:
        full, st_full = call(Xd, Hd, win)
        got, st = call(Xp, Hp, win[cells])
        assert got.shape == full.shape[:2] + (Gq,), name
        assert int(st.item()) == int(st_full.item()) == 0, name
        for k in range(full.shape[0]):
            np.testing.assert_array_equal(_bits(got[k]), _bits(full[k].index_select(1, idx)), err_msg="%s, plane %d" % (name, k))
        assert (got[:, 1] == 0).all(), name                                       # the empty period
    # the default workspace: still the full field's columns within the sum tolerance of tests/test_gpu_periods.py
    full, _ = engine.edd_ladder_reduce(Xd, Hd, rb, rows, KELVIN, THR9, doy=doy, windows=win)
    got, _ = engine.edd_ladder_reduce(Xp, Hp, rb, rows, KELVIN, THR9, doy=doy, windows=win[cells])
    np.testing.assert_allclose(got.cpu().numpy(), full.index_select(2, idx).cpu().numpy(), rtol=2e-7 if dtype == np.float32 else 1e-13, atol=1e-30)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nlat,nlon", GRIDS)
def test_compact_apply_equals_the_plain_apply_of_the_scattered_rows(torch_cuda, nlat, nlon, dtype):
    """apply(compact=True) on packed rows == the plain apply of those rows scattered back into a zero (rows, G) field, bit for
    bit: 1, 36 (a nine-threshold ladder of four periods) and 70 rows (more than one time block), NaN among them, packed rows
    that are the left half of a two-field matrix, pitched rows; the region without weight is NaN in both."""
    torch = torch_cuda
    c = _Sparse(nlat, nlon, dtype, seed=nlat + 2)
    plan = c.plan()
    cells = plan.compact_cells(dtype)
    Gq = len(cells)
    rng = np.random.default_rng(7)
    for n_rows in (1, 36, 70):
        P = (1000 * rng.standard_normal((n_rows, Gq))).astype(dtype)
        P[rng.uniform(size=P.shape) < 0.01] = np.nan
        S = np.zeros((n_rows, c.G), dtype=dtype)
        S[:, cells] = P
        want = plan.apply(torch.from_numpy(S).cuda())
        assert tuple(want.shape) == (n_rows, c.R) and bool(torch.isnan(want[:, c.R - 1]).all())
        two = torch.from_numpy(np.concatenate([P, -P], axis=1)).cuda()
        for name, Pd in (("contiguous", torch.from_numpy(P).cuda()), ("left half of two fields", two[:, :Gq]),
                         ("pitched by 3 elements", _strided(torch, P, 3))):
            got = plan.apply(Pd, compact=True)
            np.testing.assert_array_equal(_bits(got), _bits(want), err_msg="%d rows, %s" % (n_rows, name))
    plan.status()
    with pytest.raises(ValueError):
        plan.apply(torch.from_numpy(P[:, :Gq - 4]).cuda(), compact=True)
    with pytest.raises(ValueError):
        plan.apply(torch.from_numpy(P).cuda(), compact=True, out_layout="RT")


def test_plans_without_a_compact_row_are_unsupported_not_emulated(torch_cuda):
    """WAGG_PLAN_NO_LINES and many-plans have no compact row (Gq = 0); pack_rows and apply(compact=True) raise, and the raw
    descriptor bit is WAGG_EUNSUPPORTED for them, for a dense-family plan, for (gridcell, time) data and for a transform."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    c = _Sparse(16, 32, np.float32, seed=5)
    X = torch.from_numpy(c.tas.reshape(T, c.G)).cuda()
    no_lines = c.plan(flags=_lib.PLAN_NO_LINES)
    assert no_lines.compact_cells(np.float32) is None and no_lines.compact_cells(np.float64) is None
    with pytest.raises(engine.WaggError):
        engine.pack_rows(no_lines, X)
    with pytest.raises(engine.WaggError):
        no_lines.apply(X, compact=True)
    many = engine.ManyPlan(c.cell, c.code, [c.w_eff, c.w_eff], c.G, c.R, row_len=c.nlon)
    gq = _lib.C.c_int64(-1)
    _lib.check(_lib.load().wagg_plan_compact_info(many._h, 4, _lib.C.byref(gq)), "wagg_plan_compact_info")
    assert gq.value == 0
    good = c.plan()
    out = torch.empty((T, c.R), dtype=torch.float32, device="cuda")
    dense = engine.DensePlan.from_segments(c.cell, c.code, c.w_eff, c.G, c.R)
    base = dict(elem=_lib.T_F32, source=_lib.SRC_DEVICE, x=X.data_ptr(), T=T, ldx=c.G, out=out.data_ptr(), ldo=c.R,
                flags=_lib.APPLY_COMPACT_ROWS)
    for what, fields in (("no lines", dict(plan_kind=_lib.PLAN_SEGMENT, plan=no_lines._h)),
                         ("many", dict(plan_kind=_lib.PLAN_SEGMENT, plan=many._h, ldo=2 * c.R)),
                         ("dense", dict(plan_kind=_lib.PLAN_DENSE, plan=dense._h)),
                         ("GT", dict(plan_kind=_lib.PLAN_SEGMENT, plan=good._h, layout=_lib.LAYOUT_GT)),
                         ("RT", dict(plan_kind=_lib.PLAN_SEGMENT, plan=good._h, out_layout=_lib.OUT_RT)),
                         ("poly", dict(plan_kind=_lib.PLAN_SEGMENT, plan=good._h, transform=_lib.XF_POLY, offset=0.0, pow_first=1, n_pow=1)),
                         ("host", dict(plan_kind=_lib.PLAN_SEGMENT, plan=good._h, source=_lib.SRC_HOST))):
        with pytest.raises(engine.WaggError) as e:
            _lib.run(what, **dict(base, **fields))
        assert e.value.code == _lib.EUNSUPPORTED, what


# ---------------------------------------------------------------------------------------------------------------------
# host-resident fields
# ---------------------------------------------------------------------------------------------------------------------
def _big_table(nlat, nlon, seed):
    """``(cell, code, weight, G, R)``: 30 % of the quads, regions = blocks of 8 rows x 32 columns (compact, like real regions)"""
    rng = np.random.default_rng(seed)
    G = nlat * nlon
    quads = np.sort(rng.choice(G // 4, size=int(0.3 * (G // 4)), replace=False))
    cells = (4 * quads[:, None] + np.arange(4)[None, :]).reshape(-1)
    cells = cells[rng.uniform(size=len(cells)) < 0.9]
    code = (cells // nlon // 8) * (nlon // 32) + (cells % nlon) // 32
    return cells.astype(np.int32), code.astype(np.int32), rng.uniform(0.1, 1.0, len(cells)), G, (nlat // 8) * (nlon // 32)


def test_pack_rows_from_host_arrays_ships_the_quads_only(torch_cuda):
    """Just above the gather threshold (fp32, T = 32, 512 x 1024 cells: 64 MiB a field), two fields: pack_rows from host arrays
    == the device pack bit for bit, through the gather (PACK_STATS["host"]), and what crossed PCIe was packed rows: more than
    nothing, at most 80 % of the fields' bytes."""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    nlat, nlon, Tn = 512, 1024, 32
    cell, code, w, G, R = _big_table(nlat, nlon, seed=1)
    plan = engine.SparsePlan(cell, code, w, G, R, row_len=nlon)
    cells = plan.compact_cells(np.float32)
    assert cells is not None and 5 * len(cells) <= 4 * G
    rng = np.random.default_rng(2)
    X = rng.standard_normal((Tn, G), dtype=np.float32)
    H = X + rng.uniform(0, 12, X.shape).astype(np.float32)
    assert X.nbytes >= 64 << 20
    want = engine.pack_rows(plan, torch.from_numpy(X).cuda(), torch.from_numpy(H).cuda())
    before = dict(engine.PACK_STATS)
    _lib.host_stats(reset=True)
    got = engine.pack_rows(plan, X, H)
    st = _lib.host_stats()
    print("host pack: lines_h2d_bytes = %d of %d field bytes (%.1f %%); PACK_STATS %r -> %r"
          % (st["lines_h2d_bytes"], X.nbytes + H.nbytes, 100.0 * st["lines_h2d_bytes"] / (X.nbytes + H.nbytes), before, engine.PACK_STATS))
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert st["lines_h2d_bytes"] > 0
    assert st["lines_h2d_bytes"] <= 0.8 * (X.nbytes + H.nbytes)
    assert st["lines_h2d_bytes"] == got.numel() * 4 and st["direct_d2h_bytes"] == 0 and st["staged_d2h_bytes"] == 0
    assert engine.PACK_STATS["host"] == before["host"] + 1 and engine.PACK_STATS["host_fallback"] == before["host_fallback"]
    one = engine.pack_rows(plan, X)
    np.testing.assert_array_equal(_bits(one), _bits(want[:, :len(cells)]))


def test_small_host_arrays_fall_back_to_upload_and_device_pack(torch_cuda):
    """1 MiB a field is below the gather threshold: host_fallback, nothing packed on the host, the same bits"""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    nlat, nlon, Tn = 64, 128, 32
    cell, code, w, G, R = _big_table(nlat, nlon, seed=3)
    plan = engine.SparsePlan(cell, code, w, G, R, row_len=nlon)
    rng = np.random.default_rng(4)
    X = rng.standard_normal((Tn, G), dtype=np.float32)
    H = X + 1
    assert X.nbytes == 1 << 20
    want = engine.pack_rows(plan, torch.from_numpy(X).cuda(), torch.from_numpy(H).cuda())
    before = dict(engine.PACK_STATS)
    _lib.host_stats(reset=True)
    got = engine.pack_rows(plan, X, H)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert _lib.host_stats()["lines_h2d_bytes"] == 0
    assert engine.PACK_STATS["host_fallback"] == before["host_fallback"] + 1 and engine.PACK_STATS["host"] == before["host"]


# ---------------------------------------------------------------------------------------------------------------------
# cells="referenced" of the public calls
# ---------------------------------------------------------------------------------------------------------------------
def _celsius(ds):
    from climate_toolbox_amd.transformations import convert_kelvin_to_celsius
    for k in ("tasmin", "tasmax"):
        ds[k].attrs["units"] = "K"
        ds = convert_kelvin_to_celsius(ds, k)
    return ds


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    assert (np.isnan(a) == np.isnan(b)).all()
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300))) if ok.any() else 0.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nlat,nlon", GRIDS)
def test_referenced_cells_match_the_oracles(torch_cuda, segment_plans, nlat, nlon, dtype):
    """cells="referenced" against the fp64 oracles of tests/test_gpu_seasons.py / test_gpu_edd_ladder.py at the project's
    tolerances: season totals of a plain variable and of a degree-day variable, tas_poly powers 1..4 with a season, a
    nine-threshold ladder with and without a season, a plain annual total -- device-resident, host-resident and (lat, lon, time)
    fields.  NaN and +-inf in cells of quads that no row reads change nothing, where cells="all" raises on them -- quads outside
    the compact row, that is: besides the referenced quads it holds the first quad of every whole-line chunk (the consumers'
    padding lanes read it with weight 0), so those few stay visible to the +-inf status.  Every call packed (PACK_STATS) -- none
    fell back.  The largest relative difference to cells="all" is printed per case."""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import engine, minixr, periods
    from climate_toolbox_amd.transformations import snyder_edd, snyder_edd_aggregate, tas_poly_aggregate
    from oracle import ref_numpy as O
    torch = torch_cuda
    c = _Sparse(nlat, nlon, dtype, seed=nlat + 3)
    c.time = np.datetime64("2003-12-12") + np.arange(T)                           # 20 days of 2003, 20 of 2004
    gd, z1, z2 = _seasons_for(c, seed=T)
    sw = pkg.season_windows(gd)
    lab = np.repeat([0, 1, 2], [5, 13, 22])
    lab[7] = -1
    labels, rb, rows = periods.period_rows(c.time, lab)
    ylabels, yrb, yrows = periods.period_rows(c.time, "year")
    mask = _mask_TG(z1, z2, pkg.day_of_year(c.time))
    assert np.isnan(mask).any() and (mask == 0).any() and (mask == 1).any()
    cmin, cmax = c.tas + dtype(KELVIN), c.tasmax + dtype(KELVIN)
    e_own = float(cmin[0].reshape(-1)[c.cell[1]])
    thr = [e_own if e == 1.5 else e for e in THR9]
    tag = "%dx%d %s" % (nlat, nlon, np.dtype(dtype).name)
    packs = lambda: engine.PACK_STATS["device"] + engine.PACK_STATS["host"] + engine.PACK_STATS["host_fallback"]
    in_row = c.plan().compact_cells(dtype)
    assert in_row is not None and np.isin(c.cell, in_row).all()

    def dataset(device=True, moved=False, poison=False):
        f = {k: (c.poisoned(v, in_row) if poison else v) for k, v in (("tas", c.tas), ("tasmin", c.tas), ("tasmax", c.tasmax))}
        if poison:                                                                # (tasmin <= tasmax is checked everywhere)
            f["tasmax"] = np.where(np.isinf(f["tasmin"]), f["tasmin"], f["tasmax"])
        if not moved:
            return _celsius(c.dataset(torch, device=device, **f))
        wrap = (lambda v: torch.from_numpy(v).cuda()) if device else (lambda v: v)
        return _celsius(minixr.Dataset({k: (("lat", "lon", "time"), wrap(np.ascontiguousarray(np.moveaxis(v, 0, -1)))) for k, v in f.items()},
                                       coords={"time": c.time, "lat": c.lat, "lon": c.lon}))

    def both(call, name):
        """the call with cells="referenced" (which must pack) and with "all"; prints their largest relative difference"""
        n0 = packs()
        got = call("referenced")
        assert packs() > n0, name
        n0 = packs()
        old = call("all")
        assert packs() == n0, name
        print("%s, %s: referenced vs all, max rel diff %.3g" % (tag, name, max(_rel(g, o) for g, o in zip(got, old))))
        return got

    # season totals: a plain variable and a degree-day variable
    ds = dataset()
    ds["edd"] = snyder_edd(ds.tasmin, ds.tasmax, e_own)
    for name, f in (("tas", c.tas), ("edd", O.snyder_edd_values(cmin, cmax, e_own))):
        ref, absref = _oracle(c, mask * np.asarray(f).reshape(T, c.G), rb, rows)
        if name != "tas":
            absref = np.maximum(absref, 0.05 * T)
        got, = both(lambda cells: [pkg.weighted_aggregate_grid_to_regions_periods(ds, name, "popwt", "reg", c.df, period=lab, season=sw,
                                                                                   cells=cells)[name].values], "season totals of " + name)
        assert got.dtype == dtype and got.shape == (3, c.R) and np.isnan(got[:, c.R - 1]).all() and np.isnan(ref[:, c.R - 1]).all()
        _ok(got, ref, c.rtol, absref)
    # tas_poly powers 1..4 with a season (the reference's tas_poly numbers the days of a call 1 .. T: those are its days of year)
    pmask = _mask_TG(z1, z2, np.arange(1, T + 1))
    call = lambda cells, d=None: [tas_poly_aggregate(d or c.dataset(torch), [1, 2, 3, 4], "popwt", "reg", c.df, period=lab, season=sw, cells=cells)[
        "tas-poly-%d" % p].values for p in (1, 2, 3, 4)]
    got = both(call, "tas_poly 1..4 with a season")
    for p in (1, 2, 3, 4):
        ref, absref = _oracle(c, pmask * O.tas_poly_values(c.tas, p).reshape(T, c.G), rb, rows)
        _ok(got[p - 1], ref, c.rtol, absref)
    # a nine-threshold ladder, annual totals, with and without a season
    for season, m in ((sw, mask), (None, 1.0)):
        name = "ladder of 9, annual" + (", season" if season is not None else "")
        ladder = lambda cells, d=None: list(snyder_edd_aggregate(d or dataset(), thr, "popwt", "reg", c.df, period="year", season=season,
                                                                 cells=cells)["edd"].values)
        got = both(ladder, name)
        for k, e in enumerate(thr):
            ref, absref = _oracle(c, m * np.asarray(O.snyder_edd_values(cmin, cmax, e)).reshape(T, c.G), yrb, yrows)
            _ok(got[k], ref, c.rtol, np.maximum(absref, 0.05 * T))
        # host-resident and (lat, lon, time) fields: the same kernels on the same numbers
        np.testing.assert_array_equal(np.stack(ladder("referenced", dataset(device=False))), np.stack(got))
        moved = snyder_edd_aggregate(dataset(moved=True), thr, "popwt", "reg", c.df, period="year", season=season, cells="referenced")
        assert moved["edd"].dims == ("refTemp", "reg", "period")
        np.testing.assert_array_equal(np.swapaxes(moved["edd"].values, 1, 2), np.stack(got))
        # NaN and +-inf in quads no row reads: nothing changes
        np.testing.assert_array_equal(np.stack(ladder("referenced", dataset(poison=True))), np.stack(got))
    with pytest.raises(ValueError):                                               # (cells="all" sees the ocean's +-inf)
        snyder_edd_aggregate(dataset(poison=True), thr, "popwt", "reg", c.df, period="year")
    # a plain annual total: sum first, whatever the automatic route would be
    ref, absref = c.oracle(c.tas, yrb, yrows)
    got, = both(lambda cells: [pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch), "tas", "popwt", "reg", c.df, period="year",
                                                                               cells=cells).tas.values], "annual total")
    np.testing.assert_array_equal(labels, [0, 1, 2])
    assert list(ylabels) == [2003, 2004] and got.shape == (2, c.R)
    _ok(got, ref, c.rtol, absref)
    n0 = packs()
    host = pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch, device=False), "tas", "popwt", "reg", c.df, period="year",
                                                          cells="referenced").tas.values
    assert packs() == n0 + 1
    np.testing.assert_array_equal(host, got)
    with pkg.results_on_device():
        on = pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch), "tas", "popwt", "reg", c.df, period="year", cells="referenced")
        assert isinstance(on.tas.data, torch.Tensor) and on.tas.data.is_cuda
    np.testing.assert_array_equal(on.tas.values, got)


@pytest.mark.parametrize("kind", ["dense", "no lines"])
def test_plans_without_the_quads_map_fall_back_to_all_cells(torch_cuda, monkeypatch, kind):
    """a dense-family plan and a WAGG_PLAN_NO_LINES plan: cells="referenced" packs nothing and equals cells="all" bit for bit"""
    import climate_toolbox_amd as pkg
    from climate_toolbox_amd import _lib, _plans, engine
    from climate_toolbox_amd.transformations import snyder_edd_aggregate, tas_poly_aggregate
    torch = torch_cuda
    pkg.clear_caches()
    monkeypatch.setattr(_plans, "_wants_dense", lambda n_ucells, G, layout, **k: kind == "dense" and layout == "TG")
    if kind == "no lines":
        real = _plans.SparsePlan
        monkeypatch.setattr(_plans, "SparsePlan", lambda *a, **k: real(*a, **dict(k, flags=_lib.PLAN_NO_LINES)))
    c = _Sparse(16, 32, np.float32, seed=11)
    gd, z1, z2 = _seasons_for(c, seed=T)
    sw = pkg.season_windows(gd)
    before = dict(engine.PACK_STATS)
    try:
        for cells_call in (lambda cells: tas_poly_aggregate(c.dataset(torch), [1, 2], "popwt", "reg", c.df, period="year", season=sw, cells=cells)["tas-poly-2"].values,
                           lambda cells: snyder_edd_aggregate(_celsius(c.dataset(torch, tasmin=c.tas, tasmax=c.tasmax)), THR9, "popwt", "reg", c.df,
                                                              period="year", cells=cells)["edd"].values,
                           lambda cells: pkg.weighted_aggregate_grid_to_regions_periods(c.dataset(torch, device=False), "tas", "popwt", "reg", c.df,
                                                                                        period="year", cells=cells).tas.values):
            np.testing.assert_array_equal(_bits(cells_call("referenced")), _bits(cells_call("all")))
        assert engine.PACK_STATS == before
        kinds = {type(p).__name__ for p in _plans._PLAN_CACHE.values()}
        assert kinds == ({"DensePlan"} if kind == "dense" else {"SparsePlan"}), kinds
    finally:
        pkg.clear_caches()
