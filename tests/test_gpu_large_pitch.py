"""Row offsets beyond 2 GiB, 4 GiB and 2^31 elements: every kernel family of csrc/ on small shapes whose rows lie gigabytes
apart (tests/large_pitch.py: one sentinel-filled buffer, a lead in front of row 0, rows `pitch` elements apart), so that an
address whose row offset lost a bit at 32 reads sentinel or a foreign row -- a wrong number, never a fault.

Tier "bytes" (A): the last two rows start 2^32 bytes or more from the view's base; tier "elems" (B): 2^31 elements or more.
Every case makes two comparisons: the bits of the same plan or call on a small copy of the same data with the same alignment
class (the contiguous copy where that has the view's class, else the copy padded by a few elements -- the kernel is then the
same), and the fp64 reference the small-shape module of that family uses, at that module's own tolerance.  Results go into a
window of a buffer filled with 12345.0 whose border must come back untouched.

  a  segment table, (time, gridcell): routes F / A / C / D of tests/test_gpu_fallback_routes.py (sparse_lcv_kernel on whole
     lines and on region-shaped chunks, sparse_stream_kernel, sparse_gather_kernel, the giant arm beside each), T = 6 and 70
  b  segment table, (gridcell, time): 1440 cell rows a pitch apart
  c  results with a large ldo / region pitch / plane stride, through the descriptor (wagg_apply)
  d  ManyPlan
  e  dense family: every VARIANT of tests/test_gpu_dense_forms_small.py, packed and pack-free passes
  f  row-list reductions: period, season, ladder, bins; aligned and element-wise kernels; pitched results
  g  engine.pack_rows
  h  the element kernels of csrc/wagg_util.hip on 2^31 + 4096 elements

LAYOUTS lists the layout of every big buffer of every case; tests/test_large_pitch_host.py checks them without a GPU, and
`_Bigs.place` refuses a layout that is not listed."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import large_pitch as LP
from tests import test_gpu_dense_forms_small as DF
from tests import test_gpu_fallback_routes as FR
from tests import test_gpu_many_small as MS
from tests.test_gpu_bins import _exact, _restate
from tests.test_gpu_packed_totals import THR9
from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok, torch_cuda  # noqa: F401  (torch_cuda: the parity tests' fixture)
from tests.test_gpu_periods import SUM_TOL, _ok, _psum
from tests.test_gpu_seasons import KELVIN, _doys, _mixed_cells, _pack
from tests.test_seasons_host import ref_mask

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
DT_IDS = ["f32", "f64"]
EB = {F32: 4, F64: 8}
RTOL = {F32: RTOL32, F64: RTOL64}
SENTINEL = 12345.0
TIER_ID = {"bytes": "A", "elems": "B"}

# (case id, rows, cols, elem_bytes, tier, aligned, planes) of every big buffer
LAYOUTS = []


def _reg(case, rows, cols, dtype, tier, aligned=True, planes=1):
    LAYOUTS.append((case, int(rows), int(cols), EB[dtype], tier, bool(aligned), int(planes)))


def _listed():
    return {c[1:] for c in LAYOUTS}


# ---- big buffers ---------------------------------------------------------------------------------------------------------------
def _aligned(v):
    return v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0


class _Bigs:
    """The big buffers of one case.  Rows are written and read back through 1-D slices of the buffer (their addresses are
    64-bit host arithmetic), not through the strided view."""

    def __init__(self, torch):
        self.torch, self.bytes = torch, 0

    def alloc(self, rows, cols, tdtype, tier, aligned=True, planes=1, fill=LP.X_SENTINEL):
        torch = self.torch
        eb = torch.empty(0, dtype=tdtype).element_size()
        assert (rows, cols, eb, tier, aligned, planes) in _listed(), "a layout the host test has not seen"
        lead, pitch, total = LP.layout(rows, cols, eb, tier, aligned, planes)
        self.bytes += total * eb
        if torch.cuda.mem_get_info()[1] < 2 * self.bytes:
            pytest.skip("the device holds less than twice the %.1f GiB this case needs" % (self.bytes / LP.GIB))
        return torch.full((total,), fill, dtype=tdtype, device="cuda"), lead, pitch

    def place(self, small, tier, aligned=True):
        """(buffer, view): `small` (2-D device tensor) as a view with a large pitch inside a sentinel-filled buffer"""
        T, G = small.shape
        buf, lead, pitch = self.alloc(T, G, small.dtype, tier, aligned)
        for r in range(T):
            buf[lead + r * pitch:lead + r * pitch + G] = small[r]
        v = LP.view(self.torch, buf, T, G, lead, pitch)
        assert v.stride(0) == pitch and _aligned(v) == aligned and v.data_ptr() == buf.data_ptr() + lead * buf.element_size()
        return buf, v


@pytest.fixture
def bigs(torch_cuda):
    yield _Bigs(torch_cuda)
    gc.collect()
    torch_cuda.cuda.synchronize()
    torch_cuda.cuda.empty_cache()


def _release(torch):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _twin(torch, small, aligned):
    """The small copy with the view's alignment class: `small` itself where it has it, else `small` with rows padded to the
    next pitch of that class.  The pad holds what lies behind a row of the big view, the sentinel: a vector load may fetch
    elements behind the last one of a row (never used), and a kernel that takes another arm when it sees NaN there would
    otherwise add in another order."""
    if small.shape[0] > 1 and _aligned(small) == aligned:
        return small
    T, G = small.shape
    q = 16 // small.element_size()
    pitch = -(-G // q) * q + q if aligned else G + 1 + ((G + 1) % q == 0)
    wide = torch.full((T, pitch), LP.X_SENTINEL, dtype=small.dtype, device="cuda")
    wide[:, :G] = small
    v = wide[:, :G]
    assert _aligned(v) == aligned
    return v


def _segments(buf, starts, n):
    """the window of a big result buffer (segments of n elements at `starts`), stacked; the window is refilled with the
    sentinel, after which the WHOLE buffer must hold nothing else"""
    torch = __import__("torch")
    got = torch.stack([buf[s:s + n].clone() for s in starts])
    for s in starts:
        buf[s:s + n] = SENTINEL
    step = 1 << 28
    for i in range(0, buf.numel(), step):
        assert bool((buf[i:i + step] == SENTINEL).all()), "written outside the result's window, near element %d" % i
    return got


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- a / b / c / g: the segment table --------------------------------------------------------------------------------------------
SEG_GRID = (40, 36)
SEG_G = SEG_GRID[0] * SEG_GRID[1]
SEG_CASES = [(r, T, "bytes", True) for r in "FACD" for T in (6, 70)] + [(r, 6, "elems", True) for r in "FD"] + \
            [("F", T, "bytes", False) for T in (6, 70)]
SEG_IDS = ["%s-T%d-%s%s" % (r, T, TIER_ID[tier], "" if al else "-unaligned") for r, T, tier, al in SEG_CASES]
for _i, (_r, _T, _tier, _al) in zip(SEG_IDS, SEG_CASES):
    for _dt in DTYPES:
        _reg("a-" + _i, _T, SEG_G, _dt, _tier, _al)
GT_T = 65
for _dt in DTYPES:
    _reg("b", SEG_G, GT_T, _dt, "bytes")


@pytest.fixture(scope="module")
def seg_ctx(torch_cuda):
    c = FR._Ctx(torch_cuda)
    yield c
    c.close()


def _seg_compare(ctx, bigs, plan, what, smalls, extra, layout, tier, aligned, refs, dtype):
    """one call on the big views of `smalls` and on their twins: the same bits, every plane against its reference"""
    torch = ctx.torch
    R = FR._table(*SEG_GRID).R
    held = [bigs.place(s, tier, aligned) for s in smalls]
    got = FR._apply(ctx, plan, what, tuple(v for _, v in held) + extra, layout, "TR", R)
    want = FR._apply(ctx, plan, what, tuple(_twin(torch, s, aligned) for s in smalls) + extra, layout, "TR", R)
    np.testing.assert_array_equal(got, want)
    assert len(refs) == len(got)
    for g, (ref, scale) in zip(got, refs):
        FR._check(g, ref, dtype, scale)
    del held
    _release(torch)
    bigs.bytes = 0


def _seg_calls(ctx, dtype, T, layout, plain_only):
    """(what, small fields, extra arguments, [(reference, scale)]) of the three calls of a segment-table case"""
    X = ctx.X(SEG_GRID, dtype, T, layout)
    calls = [("plain", (X,), (), [(FR._ref(*SEG_GRID, dtype, T), 1.0)])]
    if not plain_only:
        calls.append(("poly", (X,), (1, 3), [(FR._ref(*SEG_GRID, dtype, T, p), 10.0 ** p) for p in (1, 2, 3)]))
        thr = FR.THRESHOLDS[3]
        calls.append(("edd", ctx.edd(SEG_GRID, dtype, T, layout), (thr,), [(FR._ref_edd(*SEG_GRID, dtype, T, e), 0.05) for e in thr]))
    return calls


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route,T,tier,aligned", SEG_CASES, ids=SEG_IDS)
def test_segment_table_time_gridcell(seg_ctx, bigs, route, T, tier, aligned, dtype):
    """`X + (t0 + tc) * ldx + cell0` and its kin: plain, three fused powers and degree days at three thresholds (tasmax in a
    second big buffer) on rows 2^32 bytes apart and more; T = 70 starts a second 64-row block at t0 = 64.  Tier B: plain."""
    plan = seg_ctx.plan(SEG_GRID, route)
    for what, smalls, extra, refs in _seg_calls(seg_ctx, dtype, T, "TG", tier == "elems"):
        _seg_compare(seg_ctx, bigs, plan, what, smalls, extra, "TG", tier, aligned, refs, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route", ["F", "D"])
def test_segment_table_gridcell_time(seg_ctx, bigs, route, dtype):
    """`X[cell * ldx + t0 + lane]`: 1440 cell rows of 65 timesteps, the last cells 2^32 bytes and more from the first"""
    plan = seg_ctx.plan(SEG_GRID, route)
    for what, smalls, extra, refs in _seg_calls(seg_ctx, dtype, GT_T, "GT", False):
        _seg_compare(seg_ctx, bigs, plan, what, smalls, extra, "GT", "bytes", True, refs, dtype)


OUT_T = 6
OUT_R = FR._table(*SEG_GRID).R
OUT_KINDS = ["TR", "RT", "planes"]
for _dt in DTYPES:
    _reg("c-TR", OUT_T, OUT_R, _dt, "bytes")
    _reg("c-RT", OUT_R, OUT_T, _dt, "bytes")
    _reg("c-planes", OUT_T, OUT_R, _dt, "bytes", planes=3)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", OUT_KINDS)
def test_pitched_results_through_the_descriptor(seg_ctx, bigs, kind, dtype):
    """wagg_apply with a hand-filled descriptor, route F, T = 6: (time, region) rows a tier-A ldo apart, (region, time) rows
    a tier-A pitch apart, and three power planes out_pstride = T ldo apart -- the bits of the contiguous results, and not
    one element of the buffer outside the window touched."""
    from climate_toolbox_amd import _lib, engine
    torch = seg_ctx.torch
    plan = seg_ctx.plan(SEG_GRID, "F")
    X = seg_ctx.X(SEG_GRID, dtype, OUT_T)
    T, R = OUT_T, OUT_R
    rows, cols, planes = (R, T, 1) if kind == "RT" else (T, R, 3 if kind == "planes" else 1)
    buf, lead, pitch = bigs.alloc(rows, cols, X.dtype, "bytes", planes=planes, fill=SENTINEL)
    fields = dict(plan_kind=_lib.PLAN_SEGMENT, plan=plan._h, elem=_lib.T_F64 if dtype == F64 else _lib.T_F32, source=_lib.SRC_DEVICE,
                  x=X.data_ptr(), T=T, ldx=SEG_G, layout=_lib.LAYOUT_TG, out=buf.data_ptr() + lead * buf.element_size(), ldo=pitch,
                  out_layout=_lib.OUT_RT if kind == "RT" else _lib.OUT_TR, stream=engine._stream_handle(None))
    if kind == "planes":
        fields.update(transform=_lib.XF_POLY, offset=FR.OFFSET, pow_first=1, n_pow=3, out_pstride=T * pitch)
        assert T * pitch * EB[dtype] > 1 << 32
        want = plan.apply_poly(X, FR.OFFSET, 3)
    else:
        want = plan.apply(X, out_layout=kind)
    _lib.run("wagg_apply", **fields)
    got = _segments(buf, [lead + i * pitch for i in range(planes * rows)], cols).reshape(want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    got = got.cpu().numpy()
    refs = [(p, 10.0 ** p) for p in (1, 2, 3)] if kind == "planes" else [(0, 1.0)]
    for g, (p, scale) in zip(got if kind == "planes" else [got], refs):
        FR._check(g.T if kind == "RT" else g, FR._ref(*SEG_GRID, dtype, T, p), dtype, scale)


PACK_CASES = [(F32, "bytes"), (F32, "elems"), (F64, "bytes")]
PACK_T = 6
for _dt, _tier in PACK_CASES:
    _reg("g-%s-%s" % (np.dtype(_dt).name, TIER_ID[_tier]), PACK_T, SEG_G, _dt, _tier)


@pytest.mark.parametrize("dtype,tier", PACK_CASES, ids=["%s-%s" % (i, TIER_ID[t]) for (_, t), i in zip(PACK_CASES, ("f32", "f32", "f64"))])
def test_pack_rows(seg_ctx, bigs, dtype, tier):
    """`src + (r + u) * ldx` of csrc/wagg_pack.hip, one field and two: X[:, compact_cells] bit for bit"""
    from climate_toolbox_amd import engine
    torch = seg_ctx.torch
    plan = seg_ctx.plan(SEG_GRID, "F")
    cells = plan.compact_cells(dtype)
    assert cells is not None and 0 < len(cells) <= SEG_G
    idx = torch.from_numpy(np.asarray(cells, dtype=np.int64)).cuda()
    lo, hi = seg_ctx.edd(SEG_GRID, dtype, PACK_T)
    X = seg_ctx.X(SEG_GRID, dtype, PACK_T)
    _, v = bigs.place(X, tier)
    np.testing.assert_array_equal(_bits(engine.pack_rows(plan, v)), _bits(X[:, idx]))
    np.testing.assert_array_equal(_bits(engine.pack_rows(plan, X)), _bits(X[:, idx]))
    del v, _
    _release(torch)
    bigs.bytes = 0
    (_, vlo), (_, vhi) = bigs.place(lo, tier), bigs.place(hi, tier)
    np.testing.assert_array_equal(_bits(engine.pack_rows(plan, vlo, vhi)), _bits(torch.cat([lo[:, idx], hi[:, idx]], dim=1)))


# ---- d: many plans -----------------------------------------------------------------------------------------------------------------
MANY_T, MANY_K, MANY_L = 70, 2, 1
_reg("d", MANY_T, SEG_G, F32, "bytes")


def test_many_plan(torch_cuda, bigs):
    """Two weightings x two levels (the fine one and ISO) from one pass over rows 2^32 bytes apart: every plane the bits of
    the contiguous apply and within RTOL32 of the oracle, inside a sentinel border"""
    torch = torch_cuda
    ctx = MS._Ctx(torch)
    try:
        t = MS._table(*SEG_GRID)
        many = MS._fused_plan(ctx.many(SEG_GRID, MANY_K, MANY_L))
        X = ctx.X(SEG_GRID, F32, MANY_T, False)
        want = MS._np(many.apply(X))
        _, v = bigs.place(X, "bytes")
        block = torch.full((MANY_T + 2, many.out_cols + 2), SENTINEL, dtype=X.dtype, device="cuda")
        got = MS._np(many.apply(v, out=block[1:-1, 1:-1]))
        full = block.cpu().numpy()
        inner = np.zeros(full.shape, dtype=bool)
        inner[1:-1, 1:-1] = True
        assert (full[~inner] == SENTINEL).all() and not (full[inner] == SENTINEL).any()
        assert len(got) == MANY_L + 1 and all(len(row) == MANY_K for row in got)
        for lv in range(MANY_L + 1):
            for k in range(MANY_K):
                np.testing.assert_array_equal(got[lv][k], want[lv][k])
                _rel_ok(got[lv][k], MS._ref(*SEG_GRID, F32, MANY_T, False, lv, k), RTOL32)
        assert t.G == SEG_G
    finally:
        ctx.close()


# ---- e: the dense family -----------------------------------------------------------------------------------------------------------
DENSE_TABLE, PF_TABLE = (333, 257), (384, 689)


def _t_long(v):
    return 640 if v[1] == F32 else 320


DENSE_CASES = [(DENSE_TABLE, v, 17, "bytes") for v in DF.VARIANTS] + \
              [(DENSE_TABLE, v, _t_long(v), "bytes") for v in DF.VARIANTS if v[0] in ("full", "tiles")] + \
              [(PF_TABLE, v, _t_long(v), "bytes") for v in DF.VARIANTS if v[0] in ("full", "tiles") and v[2] != "split"] + \
              [(DENSE_TABLE, DF.VARIANTS[0], 17, "elems"), (DENSE_TABLE, DF.VARIANTS[5], 17, "elems")]
assert DF.VARIANTS[0] == ("full", F32, "split") and DF.VARIANTS[5] == ("entries", F32, "")
DENSE_IDS = ["%dx%d-%s-T%d-%s" % (g[0], g[1], DF._vid(v), T, TIER_ID[tier]) for g, v, T, tier in DENSE_CASES]
for _i, (_g, _v, _T, _tier) in zip(DENSE_IDS, DENSE_CASES):
    _reg("e-" + _i, _T, _g[0], _v[1], _tier)


@pytest.fixture(scope="module")
def dense_ctx(torch_cuda):
    c = DF._Ctx(torch_cuda)
    yield c
    c.close()


@pytest.mark.parametrize("table,v,T,tier", DENSE_CASES, ids=DENSE_IDS)
def test_dense_family(dense_ctx, bigs, table, v, T, tier):
    """`X + t * ldx` of the packing kernels and the entry-list kernel, `xsrc + r * ldxB` inside the LDS-DMA of the pack-free
    pass: zero-mean fields priced by sum |x| |w| / |den| as in tests/test_gpu_dense_forms_small.py.  The 333 x 257 table packs
    at every T (333 is no whole number of k tiles); on 384 x 689 the tile-sparse form and, with two row blocks (T = 640 /
    320), the full form read the rows where they lie (DF.pack_free, asserted)."""
    torch = dense_ctx.torch
    (G, R), (form, dtype, variant) = table, v
    plan = dense_ctx.plan(G, R, form, dtype)
    X = DF.field(G, dtype, T)
    Xd = dense_ctx.dev(X)
    assert DF.pack_free(G, dtype, form, variant, T, True) == (table == PF_TABLE)
    want = DF.run(plan, variant, _twin(torch, Xd, True)).cpu().numpy()
    _, view = bigs.place(Xd, tier)
    block = torch.full((T + 2, R + 2), SENTINEL, dtype=Xd.dtype, device="cuda")
    DF.run(plan, variant, view, out=block[1:T + 1, 1:R + 1])
    full = block.cpu().numpy()
    inner = np.zeros(full.shape, dtype=bool)
    inner[1:-1, 1:-1] = True
    assert (full[~inner] == SENTINEL).all(), "written outside the result's window"
    got = full[1:-1, 1:-1]
    np.testing.assert_array_equal(got, want)
    DF.priced_ok(got, DF.oracle(G, R, dtype, T), DF.price(X, G, R, dtype, split=variant == "split"))


# ---- f: row-list reductions --------------------------------------------------------------------------------------------------------
RL_T, RL_N = 40, 1100
RL_PERIODS = [[0, 5, 5, 17, 38], [], [39, 1, 2, 3, 38], list(range(8, 30))]      # rows 0, 38, 39; row 5 twice; an empty period
RL_RB = np.concatenate([[0], np.cumsum([len(p) for p in RL_PERIODS])]).astype(np.int64)
RL_ROWS = np.concatenate([np.asarray(p, dtype=np.int64) for p in RL_PERIODS])
RL_P = len(RL_PERIODS)
RL_EDGES = [-np.inf, -12.0, 0.0, 5.5, 11.0, 19.25, 30.0, 35.0, 40.0, np.inf]         # 9 bins: a group of 8 and one more
RL_OPS = ["period", "season", "ladder", "bins"]
RL_CASES = [(op, dt, "bytes", al) for op in RL_OPS for dt in DTYPES for al in (True, False)] + \
           [("period", F32, "elems", True), ("bins", F32, "elems", True)]
RL_IDS = ["%s-%s-%s%s" % (op, "f32" if dt == F32 else "f64", TIER_ID[tier], "" if al else "-unaligned") for op, dt, tier, al in RL_CASES]
for _i, (_op, _dt, _tier, _al) in zip(RL_IDS, RL_CASES):
    _reg("f-" + _i, RL_T, RL_N, _dt, _tier, _al)
RL_OUT_PLANES = 2
_reg("f-out", RL_P, RL_N, F32, "bytes", planes=RL_OUT_PLANES)
assert len(THR9) == 9 and len(RL_EDGES) == 10


def _rl_fields(dtype):
    """(tasmin-like X, tasmax-like H) in Kelvin, random per row; a NaN in season and a cell that is NaN on every day"""
    rng = np.random.default_rng(4011)
    X = (280 + 15 * rng.standard_normal((RL_T, RL_N))).astype(dtype)
    H = (X + rng.uniform(0, 12, X.shape)).astype(dtype)
    X[0, 0] = np.nan
    X[:, 6] = np.nan
    return X, H


def _rl_out(torch, planes, tdtype):
    block = torch.full((planes + 2, RL_P, RL_N), SENTINEL, dtype=tdtype, device="cuda")
    return block, block[1:planes + 1]


def _rl_border(block):
    assert bool((block[0] == SENTINEL).all()) and bool((block[-1] == SENTINEL).all()), "written outside the result's planes"


def _rl_season():
    doy = _doys(RL_T)[0][1]
    z1, z2 = _mixed_cells(RL_N, doy)
    return doy, _pack(z1, z2), np.nan_to_num(ref_mask(z1, z2, doy), nan=0.0).T          # m01: (T, n)


def _rl_calls(op, dtype, tier):
    """[(name, planes, call(X, H, out) -> (out, status), check(got numpy (planes, P, n), fedd))] of a row-list case; `fedd`:
    the library's elementwise degree days of the small fields (periods / ladder: their SUM_TOL reference)"""
    from climate_toolbox_amd import engine
    from oracle import ref_numpy as O
    X, H = _rl_fields(dtype)
    rb, rows, rtol = RL_RB, RL_ROWS, RTOL[dtype]
    f0 = np.nan_to_num(X, nan=0.0)
    cmin, cmax = X + dtype(KELVIN), H + dtype(KELVIN)
    calls = []
    if op == "period":
        calls.append(("none", 1, lambda x, h, o: engine.period_reduce(x, rb, rows, out=o),
                      lambda g: _ok(g[0], _psum(f0, rb, rows), SUM_TOL[dtype], _psum(np.abs(f0), rb, rows))))
        if tier == "elems":
            return calls

        def check_poly(g):
            for k in range(4):
                f = np.nan_to_num(O.tas_poly_values(X, k + 1), nan=0.0)
                _ok(g[k], _psum(f, rb, rows), rtol, _psum(np.abs(f), rb, rows))

        calls.append(("poly", 4, lambda x, h, o: engine.period_reduce(x, rb, rows, poly=(KELVIN, 1, 4), out=o), check_poly))
        thr = [float(cmin[0, 1]), 12.5, float(cmax[0, 2])]

        def check_edd(g):
            for k, e in enumerate(thr):
                o = np.nan_to_num(O.snyder_edd_values(cmin, cmax, e), nan=0.0)
                _rel_ok(g[k], _psum(o, rb, rows), rtol, scale=0.05 * RL_T)

        calls.append(("edd", 3, lambda x, h, o: engine.period_reduce(x, rb, rows, X2=h, edd=(KELVIN, thr), out=o), check_edd))
    elif op == "season":
        doy, win, m01 = _rl_season()
        calls.append(("season", 1, lambda x, h, o: engine.season_reduce(x, rb, rows, doy, win, out=o),
                      lambda g: _ok(g[0], _psum(m01 * f0, rb, rows), SUM_TOL[dtype], _psum(m01 * np.abs(f0), rb, rows))))
    elif op == "ladder":
        doy, win, m01 = _rl_season()
        oedd = np.stack([np.nan_to_num(O.snyder_edd_values(cmin, cmax, e), nan=0.0) for e in THR9], axis=1)       # (T, 9, n)
        calls.append(("ladder", 9, lambda x, h, o: engine.edd_ladder_reduce(x, h, rb, rows, KELVIN, THR9, doy=doy, windows=win, out=o),
                      lambda g: _rel_ok(np.moveaxis(g, 0, 1), _psum(m01[:, None, :] * oedd, rb, rows), rtol, scale=0.05 * RL_T)))
    else:
        want = _restate(X, np.ones_like(f0), rb, rows, RL_EDGES, KELVIN)
        calls.append(("bins", 9, lambda x, h, o: engine.bin_days_reduce(x, rb, rows, KELVIN, RL_EDGES, out=o),
                      lambda g: _exact(__import__("torch").from_numpy(g), want, "bins")))
    return calls


@pytest.mark.parametrize("op,dtype,tier,aligned", RL_CASES, ids=RL_IDS)
def test_row_list_reductions(torch_cuda, bigs, op, dtype, tier, aligned):
    """`k * pstride`, `out + p * ldo + col` and the row reads `X + row * ldx` of the row-list kernels: T = 40 rows of 1100
    cells (two column blocks), four periods (so few blocks that a list is split across blocks) that list rows 0, 38 and 39,
    one row twice, and an empty period; 16-byte aligned rows and rows one element over (the cell-by-cell kernels)."""
    torch = torch_cuda
    X, H = _rl_fields(dtype)
    Xd, Hd = torch.from_numpy(X).cuda(), torch.from_numpy(H).cuda()
    needs_h = op in ("period", "ladder") and tier != "elems"
    _, vx = bigs.place(Xd, tier, aligned)
    vh = bigs.place(Hd, tier, aligned)[1] if needs_h else None
    tx, th = _twin(torch, Xd, aligned), _twin(torch, Hd, aligned)
    for name, planes, call, check in _rl_calls(op, dtype, tier):
        block, win = _rl_out(torch, planes, Xd.dtype)
        got, st = call(vx, vh, win)
        _rl_border(block)
        want, st2 = call(tx, th, None)
        assert int(st.item()) == int(st2.item()) == 0, name
        assert torch.equal(got, want), name
        check(got.cpu().numpy())
        if op in ("period", "season"):
            assert bool((got[:, 1] == 0).all()), "the empty period totals 0"


@pytest.mark.parametrize("op", ["period", "bins"])
def test_row_list_pitched_results(torch_cuda, bigs, op):
    """The library calls themselves (the binding hands them contiguous results only): two planes whose period rows lie a
    tier-A ldo apart and whose planes P ldo apart -- the contiguous result's bits, nothing else in the buffer touched"""
    from climate_toolbox_amd import _lib, engine
    torch = torch_cuda
    X, _ = _rl_fields(F32)
    Xd = torch.from_numpy(X).cuda()
    L = _lib.load()
    c = engine._RowlistCall(Xd, RL_RB, RL_ROWS, False)
    buf, lead, ldo = bigs.alloc(RL_P, RL_N, Xd.dtype, "bytes", planes=RL_OUT_PLANES, fill=SENTINEL)
    pstride = RL_P * ldo
    assert ldo * 4 >= 1 << 31 and pstride * 4 > 1 << 32
    out_ptr = C.c_void_p(buf.data_ptr() + lead * 4)
    vp = lambda t: C.c_void_p(t.data_ptr())
    if op == "period":
        want, _ = engine.period_reduce(Xd, RL_RB, RL_ROWS, poly=(KELVIN, 1, RL_OUT_PLANES))
        _, status, work, wb = c.alloc(L.wagg_period_reduce_work_bytes, RL_OUT_PLANES, None, None)
        rc = L.wagg_period_reduce_f32(vp(Xd), None, c.T, c.n, RL_N, vp(c.row_begin), vp(c.rows), c.P, c.n_rows, _lib.XF_POLY, KELVIN, 1,
                                      RL_OUT_PLANES, None, 0, c.flags, out_ptr, ldo, pstride, vp(status), work, wb, engine._stream_handle(None))
    else:
        edges = np.ascontiguousarray([-np.inf, 11.0, np.inf])
        want, _ = engine.bin_days_reduce(Xd, RL_RB, RL_ROWS, KELVIN, edges)
        _, status, work, wb = c.alloc(lambda n, P, n_rows, planes: L.wagg_bin_days_work_bytes(n, P, n_rows, planes + 1), RL_OUT_PLANES, None, None)
        rc = L.wagg_bin_days_reduce_f32(vp(Xd), c.T, c.n, RL_N, vp(c.row_begin), vp(c.rows), c.P, c.n_rows, None, None, KELVIN,
                                        edges.ctypes.data_as(C.POINTER(C.c_double)), len(edges), c.flags, out_ptr, ldo, pstride, vp(status),
                                        work, wb, engine._stream_handle(None))
    _lib.check(rc, "row-list call with a pitched result")
    assert int(status.item()) == 0
    got = _segments(buf, [lead + i * ldo for i in range(RL_OUT_PLANES * RL_P)], RL_N).reshape(want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    if op == "bins":
        _exact(got, _restate(X, np.ones(X.shape), RL_RB, RL_ROWS, edges, KELVIN), "bins")


# ---- h: the element kernels ----------------------------------------------------------------------------------------------------------
N_ELEMS = (1 << 31) + 4096
CHUNK = 1 << 24
GATHER_T = 6
_reg("h-gather", GATHER_T, SEG_G, F32, "elems")


def _budget(torch, nbytes):
    if torch.cuda.mem_get_info()[1] < 2 * nbytes:
        pytest.skip("the device holds less than twice the %.1f GiB this case needs" % (nbytes / LP.GIB))


def _ramp(torch, n, base, amp, seed):
    """n fp32 values: one random chunk of 2^24 values, repeated with 0.125 c added in chunk c -- so elements 2^31 or 2^32
    positions apart differ by 16 or 32"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    r = base + amp * torch.rand(CHUNK, generator=g, device="cuda", dtype=torch.float32)
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    for c, i in enumerate(range(0, n, CHUNK)):
        m = min(CHUNK, n - i)
        x[i:i + m] = r[:m] + 0.125 * c
    return x


def _sliced(n):
    return [(i, min(i + CHUNK, n)) for i in range(0, n, CHUNK)]


def _close(torch, got, ref64, rtol, scale):
    """the rule of _rel_ok on the device: |got - ref| <= rtol max(|ref|, scale); `scale`: a number or a tensor"""
    err = (got.double() - ref64).abs()
    return bool((err <= rtol * torch.maximum(ref64.abs(), torch.as_tensor(scale, dtype=torch.float64, device=ref64.device))).all())


def test_element_kernels_transforms(torch_cuda, bigs):
    """wagg_transform_poly_f32 (power 3) and wagg_transform_edd_f32 on 2^31 + 4096 contiguous elements against torch's own
    fp64 arithmetic over the whole array, in slices: RTOL32 relative to terms of 10^3 for the cube (the rule of
    tests/test_gpu_fallback_routes.py for power p: terms of 10^p) and, for the degree days of ONE cell, relative to the terms
    the formula adds, |mean - e| + width (an fp32 evaluation errs by a few ulp of those; a region's average, which the 0.05 of
    the aggregation tests belongs to, does not exist here).  A slice read 2^31 elements off differs by 16 K."""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = N_ELEMS
    _budget(torch, 4 * 4 * n)
    lo = _ramp(torch, n, 280.0, 20.0, 1)
    out = engine.transform_poly(lo, KELVIN, 3)
    assert out.shape == lo.shape
    for a, b in _sliced(n):
        assert _close(torch, out[a:b], (lo[a:b].double() + float(np.float32(KELVIN))) ** 3, RTOL32, 1e3), (a, b)
    del out
    hi = _ramp(torch, n, 284.0, 28.0, 2)
    torch.maximum(hi, lo, out=hi)
    e, off = 22.0, float(np.float32(KELVIN))
    out = engine.transform_edd(lo, hi, KELVIN, [(1.0, e)])
    for a, b in _sliced(n):
        tmin, tmax = lo[a:b].double() + off, hi[a:b].double() + off
        mean, width = (tmax + tmin) / 2, (tmax - tmin) / 2
        theta = torch.arcsin(torch.clamp((e - mean) / width, -1.0, 1.0))
        inner = torch.where(tmax > e, ((mean - e) * (np.pi / 2 - theta) + width * torch.cos(theta)) / np.pi, torch.zeros_like(mean))
        ref = torch.where(tmin < e, inner, mean - e)
        assert _close(torch, out[a:b], ref, RTOL32, (mean - e).abs() + width), (a, b)


def test_element_kernels_any_less_and_combine(torch_cuda, bigs):
    """wagg_any_less_f32 with the only a < b in the LAST of 2^31 + 4096 elements, and wagg_combine_planes_f32 of two such
    planes (plane stride beyond 2^31 elements) against torch's subtraction, bit for bit"""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = N_ELEMS
    _budget(torch, 3 * 4 * n)
    stack = torch.empty((2, n), dtype=torch.float32, device="cuda")
    stack[0] = _ramp(torch, n, 280.0, 20.0, 3)
    stack[1] = stack[0]
    assert not engine.any_less(stack[0], stack[1])
    stack[0, n - 1] -= 1.0
    assert engine.any_less(stack[0], stack[1])
    assert not engine.any_less(stack[1], stack[0])
    stack[1] = _ramp(torch, n, 10.0, 5.0, 4)
    out = engine.combine_planes(stack, [1.0, -1.0])
    for a, b in _sliced(n):
        assert torch.equal(out[a:b], stack[0, a:b] - stack[1, a:b]), (a, b)


def test_element_kernels_take_axis_and_relayout(torch_cuda, bigs):
    """wagg_take_axis: rows 0 and 2 of a (3, n) array, n = 2^31 + 4096; wagg_relayout_f32: a (2, n / 2) array transposed --
    against torch's views, bit for bit"""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    n = N_ELEMS
    _budget(torch, 5 * 4 * n)
    src = torch.empty((3, n), dtype=torch.float32, device="cuda")
    for i in range(3):
        src[i] = _ramp(torch, n, 100.0 * i, 20.0, 5 + i)
    out = engine.take_axis(src, 0, [0, 2])
    assert out.shape == (2, n)
    for a, b in _sliced(n):
        assert torch.equal(out[0, a:b], src[0, a:b]) and torch.equal(out[1, a:b], src[2, a:b]), (a, b)
    del out
    two = src.reshape(-1)[:n].reshape(2, n // 2)                   # (rows of the first plane: contiguous)
    out = engine.relayout(two, [1, 0])
    assert out.shape == (n // 2, 2) and out.is_contiguous()
    for a, b in _sliced(n // 2):
        assert torch.equal(out[a:b, 0], two[0, a:b]) and torch.equal(out[a:b, 1], two[1, a:b]), (a, b)


def test_element_kernels_gather(seg_ctx, bigs):
    """wagg_gather_f32: 64 cells of every row of a tier-B view, both result layouts"""
    from climate_toolbox_amd import engine
    torch = seg_ctx.torch
    X = seg_ctx.X(SEG_GRID, F32, GATHER_T)
    _, v = bigs.place(X, "elems")
    cells = np.random.default_rng(9).choice(SEG_G, 64, replace=False).astype(np.int32)
    cells[:2] = [0, SEG_G - 1]
    idx = torch.from_numpy(cells).cuda()
    want = X[:, idx.long()]
    np.testing.assert_array_equal(_bits(engine.gather(v, idx)), _bits(want))
    np.testing.assert_array_equal(_bits(engine.gather(v, idx, out_layout="RT")), _bits(want.t().contiguous()))
