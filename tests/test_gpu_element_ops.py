"""The element and data-movement kernels of csrc/wagg_util.hip on the GPU (run with -m gpu), through engine.py and, where the
engine hides an argument, through the C-ABI: gather, transform_poly, transform_edd, any_less, combine_planes, take_axis,
relayout and to_float64, against the restatements of tests/element_ops.py (checked without a GPU in
tests/test_element_ops_host.py).

Data movement is compared as integer bit patterns over random 32- / 64-bit words with NaNs of several payloads, infinities,
-0 and subnormals planted.  Every grid-stride loop makes its second trip once per element type: the loops launch 4096 x 256
(take_axis, relayout, to_float64) or 2048 x 256 threads (transform_poly, transform_edd, any_less, combine_planes), and one
case each is just larger than that.  combine_planes is held to |got - ref| <= K eps S (derived in tests/element_ops.py,
shown to hold for a separately rounded and for a fused sum in the host module) and, with coefficients +-2^j, to the bits
of the typed left-to-right sum.  transform_poly is held to the bits of the multiplication chain in the element type."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from tests import element_ops as E

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _view(torch, flat_dev, v):
    return torch.as_strided(flat_dev, v.shape, v.strides, v.base)


def _same_bits(got, want, what):
    got = _host(got) if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    gb, wb = E.bits(got), E.bits(want)
    bad = gb != wb
    assert not bad.any(), "%s: %d of %d elements differ, first at %d: %#x for %#x" % (
        what, bad.sum(), bad.size, np.flatnonzero(bad.ravel())[0], int(gb.ravel()[np.flatnonzero(bad.ravel())[0]]),
        int(wb.ravel()[np.flatnonzero(bad.ravel())[0]]))


# ---- engine.relayout (relayout_kernel) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_relayout_is_the_address_walk(torch_cuda, dtype):
    """1 to 6 dims; identity, reversal, a swap of the outer dims, (3, 1, 0, 2); contiguous, stepped, one element into the
    buffer, an expanded dim (stride 0), dims of extent 1; an extent of 0 gives an empty result"""
    from climate_toolbox_amd import engine
    n = 0
    for v, _, _ in E.relayout_views():
        data = E.random_words(v.nbuf, dtype, 40 + n)
        t = _view(torch_cuda, _dev(torch_cuda, data), v)
        got = engine.relayout(t, v.order)
        assert got.is_contiguous()
        _same_bits(got, E.relayout_ref(data, v), v.name)
        if v.order == tuple(range(len(v.shape))):
            _same_bits(engine.relayout(t), E.relayout_ref(data, v), v.name + " (no order)")
        n += 1
    assert n > 80 and got.numel() == 0 and tuple(got.shape) == (4, 3, 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_relayout_second_trip(torch_cuda, dtype):
    """1031 x 1019 transposed: 1,050,589 elements for 1,048,576 threads"""
    from climate_toolbox_amd import engine
    v = E.big_view()
    data = E.random_words(v.nbuf, dtype, 7)
    got = engine.relayout(_view(torch_cuda, _dev(torch_cuda, data), v), v.order)
    assert got.numel() > E.GRID_WIDE
    _same_bits(got, E.relayout_ref(data, v), v.name)


def test_relayout_refusals(torch_cuda):
    from climate_toolbox_amd import engine
    torch = torch_cuda
    with pytest.raises(ValueError):
        engine.relayout(torch.zeros((1, 2, 1, 2, 1, 2, 1), dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        engine.relayout(torch.zeros((4, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        engine.relayout(torch.zeros((4, 4), dtype=torch.float32))


# ---- engine.to_float64 (relayout_to_f64_kernel<9 source types>) -------------------------------------------------------------------
def _typed(torch, kind, values):
    """the source values as a CUDA tensor of ``kind``"""
    if kind == "float16":
        return torch.from_numpy(values.view(np.float16).copy()).cuda()
    if kind == "bfloat16":
        return torch.from_numpy(values.view(np.int16).copy()).cuda().view(torch.bfloat16)
    return torch.from_numpy(values.copy()).cuda()


@pytest.mark.parametrize("kind", E.TO_F64_KINDS)
def test_to_float64_equals_the_restatement(torch_cuda, kind):
    """every 16-bit pattern / value, every 8-bit value, the extremes of int32 and int64 with the int64 values that do not fit
    53 bits, float32 and float64 words with the specials; then once from a stepped, permuted 3-D view"""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    values = E.to_f64_values(kind)
    ref = E.to_f64_ref(kind, values)
    src = _typed(torch, kind, values)
    assert str(src.dtype) == "torch." + kind and str(src.dtype) in engine._TO_F64_TYPES
    got = _host(engine.to_float64(src))
    assert got.dtype == np.float64
    why = E.same_f64(got, ref, exact_nan=kind == "float64")
    assert why is None, (kind, why)
    v = E.stepped3d()
    pick = np.arange(v.nbuf) * (len(values) // v.nbuf)
    got = _host(engine.to_float64(_view(torch, _typed(torch, kind, values[pick]), v), v.order))
    why = E.same_f64(got, E.relayout_ref(ref[pick], v), exact_nan=kind == "float64")
    assert why is None, (kind, "stepped 3-D", why)


@pytest.mark.parametrize("kind", ["uint8", "float16", "int64", "bfloat16"])
def test_to_float64_second_trip(torch_cuda, kind):
    from climate_toolbox_amd import engine
    v = E.big_view()
    values = E.to_f64_values(kind)
    cyc = np.arange(v.nbuf) % len(values)
    got = _host(engine.to_float64(_view(torch_cuda, _typed(torch_cuda, kind, values[cyc]), v), v.order))
    why = E.same_f64(got, E.relayout_ref(E.to_f64_ref(kind, values)[cyc], v))
    assert got.size > E.GRID_WIDE and why is None, (kind, why)


def test_to_float64_refusals(torch_cuda):
    from climate_toolbox_amd import engine
    torch = torch_cuda
    for dt in (torch.bool, torch.complex64):
        with pytest.raises(TypeError):
            engine.to_float64(torch.zeros(8, dtype=dt, device="cuda"))
    with pytest.raises(ValueError):
        engine.to_float64(torch.zeros((1,) * 7, dtype=torch.int16, device="cuda"))
    with pytest.raises(TypeError):
        engine.to_float64(torch.zeros(8, dtype=torch.int16))


# ---- engine.take_axis (take_axis_kernel<v4 | int>) ---------------------------------------------------------------------------------
TAKE_ROWS = [(d, b) for d in DTYPES for b in E.INNER_BYTES if E.take_shapes(d, b)]        # (no fp64 row has 4 or 12 bytes)


@pytest.mark.parametrize("dtype,inner_bytes", TAKE_ROWS, ids=["%s-inner%d" % (IDS[DTYPES.index(d)], b) for d, b in TAKE_ROWS])
def test_take_axis_equals_numpy_take(torch_cuda, dtype, inner_bytes):
    """rows of 4, 8, 12 and 24 bytes (the 4-byte kernel) and of 16, 48 and 336 bytes (the 16-byte kernel); outer 1 and 3; the
    axis first and in the middle, also counted from the end; empty, single, reversed, repeated and longer-than-the-axis lists"""
    from climate_toolbox_amd import engine
    for k, (shape, axis) in enumerate(E.take_shapes(dtype, inner_bytes)):
        a = E.random_words(int(np.prod(shape)), dtype, 60 + k).reshape(shape)
        ad = _dev(torch_cuda, a)
        for name, idx in E.index_lists(shape[axis]):
            got = engine.take_axis(ad, axis, idx)
            _same_bits(got, np.take(a, idx, axis=axis), "%r axis %d %s" % (shape, axis, name))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_take_axis_last_axis_views_and_other_dtypes(torch_cuda, dtype):
    """the last axis (rows of one element); a contiguous view that begins one element into its buffer with rows of whole
    16-byte pieces (the base is not 16-byte aligned: the 4-byte kernel serves it); a non-contiguous view; an int16 field"""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    a = E.random_words(3 * 5 * 7, dtype, 70).reshape(3, 5, 7)
    ad = _dev(torch, a)
    for axis in (2, -1):
        for name, idx in E.index_lists(7):
            _same_bits(engine.take_axis(ad, axis, idx), np.take(a, idx, axis=axis), "last axis %s" % name)
    shape = (3, 7, 48 // a.itemsize)
    n = int(np.prod(shape))
    data = E.random_words(n + 1, dtype, 71)
    view = _dev(torch, data)[1:].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0 and view.data_ptr() % a.itemsize == 0
    for name, idx in E.index_lists(7):
        _same_bits(engine.take_axis(view, 1, idx), np.take(data[1:].reshape(shape), idx, axis=1), "offset base %s" % name)
    _same_bits(engine.take_axis(ad[:, ::2, 1:6], 1, [2, 0, 1, 1]), np.take(a[:, ::2, 1:6], [2, 0, 1, 1], axis=1), "stepped view")
    i16 = np.arange(-60, 60, dtype=np.int16).reshape(4, 5, 6)
    _same_bits(engine.take_axis(_dev(torch, i16), 1, [4, 0]), np.take(i16, [4, 0], axis=1).astype(np.float64), "int16")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_take_axis_rows_of_24_bytes_with_low_indices(torch_cuda, dtype):
    """rows of one and a half 16-byte pieces, eight of them, and only the rows 0 to 2 taken: every address a kernel that took
    these rows for whole 16-byte pieces would form lies inside the source and the result, so the values alone tell the two
    kernels apart"""
    from climate_toolbox_amd import engine
    a = E.random_words(8 * 24 // np.dtype(dtype).itemsize, dtype, 73).reshape(8, -1)
    idx = [2, 0, 1, 1]
    assert a.shape[1] * a.itemsize == 24 and (8 + max(idx) + 1) * 16 <= a.nbytes
    _same_bits(engine.take_axis(_dev(torch_cuda, a), 0, idx), np.take(a, idx, axis=0), "rows of 24 bytes")


@pytest.mark.parametrize("wide", [True, False], ids=["16-byte pieces", "4-byte words"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_take_axis_second_trip(torch_cuda, dtype, wide):
    from climate_toolbox_amd import engine
    shape, axis, idx = E.take_big(dtype, wide)
    a = E.random_words(int(np.prod(shape)), dtype, 72).reshape(shape)
    got = engine.take_axis(_dev(torch_cuda, a), axis, idx)
    assert got.numel() * got.element_size() // (16 if wide else 4) > E.GRID_WIDE
    _same_bits(got, np.take(a, idx, axis=axis), "second trip")


def test_take_axis_refusals_and_host_tensors(torch_cuda):
    from climate_toolbox_amd import engine
    torch = torch_cuda
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    ad = _dev(torch, a)
    for idx in ([3], [-1], [0, 1, 2, 3], [0, -4]):
        with pytest.raises(IndexError):
            engine.take_axis(ad, 1, idx)
        with pytest.raises(IndexError):
            engine.take_axis(torch.from_numpy(a), 1, idx)
    got = engine.take_axis(torch.from_numpy(a), 2, [3, 3, 0])
    assert not got.is_cuda and np.array_equal(got.numpy(), np.take(a, [3, 3, 0], axis=2))
    with pytest.raises(TypeError):
        engine.take_axis(a, 1, [0])


# ---- engine.gather (gather_kernel) -------------------------------------------------------------------------------------------------
def _gather_field(torch, X, layout, pitched):
    """the (T, G) host matrix as the device tensor of ``layout``; ``pitched``: a column slice of a wider buffer"""
    a = X if layout == "TG" else np.ascontiguousarray(X.T)
    if not pitched:
        return _dev(torch, a)
    wide = torch.full((a.shape[0], a.shape[1] + 5), float("nan"), dtype=_dev(torch, a[:0]).dtype, device="cuda")
    wide[:, 2:2 + a.shape[1]] = _dev(torch, a)
    return wide[:, 2:2 + a.shape[1]]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_equals_numpy_indexing(torch_cuda, dtype):
    """layouts TG and GT, results TR and RT, contiguous and pitched X, T in {0, 1, 3, 70}, nseg in {0, 1, 255, 256, 257, 1000}
    (around the 256-thread block), duplicate cells, the first and the last cell of the grid"""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    G = 37 * 5
    for T in E.GATHER_T:
        X = E.random_words(T * G, dtype, 80 + T).reshape(T, G)
        for layout in ("TG", "GT"):
            for pitched in (False, True):
                Xd = _gather_field(torch, X, layout, pitched)
                assert not pitched or T == 0 or (Xd.stride(0) > Xd.shape[1] and not Xd.is_contiguous()) or Xd.shape[0] == 1
                for nseg in E.GATHER_NSEG:
                    cells = E.gather_cells(G, nseg, nseg + T)
                    cd = _dev(torch, cells)
                    for out_layout in ("TR", "RT"):
                        got = engine.gather(Xd, cd, layout=layout, out_layout=out_layout)
                        _same_bits(got, E.gather_ref(X, cells, out_layout), "T=%d %s%s nseg=%d %s" % (T, layout, " pitched" if pitched else "", nseg, out_layout))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_pitched_result_and_refusals(torch_cuda, dtype):
    """through the C-ABI: a result with ldo > nseg (TR) and ldo > T (RT) keeps a sentinel in its padding; an ldo that is too
    small and a bad layout code are refused"""
    from climate_toolbox_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    fn = L.wagg_gather_f32 if dtype == np.float32 else L.wagg_gather_f64
    T, G, nseg = 5, 64, 257
    X = E.random_words(T * G, dtype, 90).reshape(T, G)
    Xd, cells = _dev(torch, X), E.gather_cells(G, nseg, 9)
    cd = _dev(torch, cells)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(out, ldo, layout=_lib.LAYOUT_TG, out_layout=_lib.OUT_TR):
        return fn(C.c_void_p(Xd.data_ptr()), T, G, layout, C.c_void_p(cd.data_ptr()), nseg, C.c_void_p(out.data_ptr()), ldo, out_layout, stream)

    for out_layout, rows, cols in ((_lib.OUT_TR, T, nseg), (_lib.OUT_RT, nseg, T)):
        out = torch.full((rows, cols + 3), -7.5, dtype=Xd.dtype, device="cuda")
        _lib.check(call(out, cols + 3, out_layout=out_layout), "wagg_gather")
        got = _host(out)
        _same_bits(np.ascontiguousarray(got[:, :cols]), E.gather_ref(X, cells, "TR" if out_layout == _lib.OUT_TR else "RT"), "pitched result")
        assert (got[:, cols:] == -7.5).all()
        with pytest.raises(_lib.WaggError, match="ldo too small"):
            _lib.check(call(out, cols - 1, out_layout=out_layout), "wagg_gather")
    out = torch.empty((T, nseg), dtype=Xd.dtype, device="cuda")
    with pytest.raises(_lib.WaggError, match="bad layout"):
        _lib.check(call(out, nseg, layout=7), "wagg_gather")
    with pytest.raises(_lib.WaggError, match="bad out_layout"):
        _lib.check(call(out, nseg, out_layout=7), "wagg_gather")


# ---- engine.any_less (any_less_kernel) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_any_less_is_the_exact_boolean(torch_cuda, dtype):
    """n in {1, 63, 64, 65, 256, 524,289}: no hit; the only hit first, last, and at 524,288 (the first element of the second
    trip); NaN on either side, -0 < 0 and equal values are false, -inf < inf is true; non-contiguous operands; true, false,
    true in a row (a stale flag would show)"""
    from climate_toolbox_amd import engine
    torch = torch_cuda
    for n in E.ANY_LESS_N + (E.GRID_NARROW + 65,):
        a, b = np.full(n, 2, dtype), np.full(n, 1, dtype)
        a[::7] = np.nan                                                    # (NaN compares false wherever it stands)
        ad, bd = _dev(torch, a), _dev(torch, b)
        assert engine.any_less(ad, bd) is False and not E.ref_any_less(a, b)
        for at in sorted({0, n - 1, min(n - 1, E.GRID_NARROW)}):
            a2 = a.copy()
            a2[at] = 0
            assert E.ref_any_less(a2, b) and engine.any_less(_dev(torch, a2), bd) is True, (n, at)
            assert engine.any_less(ad, bd) is False, (n, at, "stale flag")
    for name, x, y, want in E.any_less_pairs(dtype):
        a, b = np.full(65, 2, dtype), np.full(65, 1, dtype)
        a[64], b[64] = x, y
        assert E.ref_any_less(a, b) == want
        assert engine.any_less(_dev(torch, a), _dev(torch, b)) is want, name
    a, b = np.full((6, 10), 2, dtype), np.full((6, 10), 1, dtype)
    a[4, 6] = 0                                                            # inside the stepped views below; a[4, 7] is not
    ad, bd = _dev(torch, a), _dev(torch, b)
    assert engine.any_less(ad[::2, ::3], bd[::2, ::3]) is True
    assert engine.any_less(ad[::2, 1::3], bd[::2, 1::3]) is False
    assert engine.any_less(ad.t(), bd.t()) is True
    with pytest.raises(ValueError):
        engine.any_less(ad, bd[:3])


# ---- engine.combine_planes (combine_planes_kernel) ---------------------------------------------------------------------------------
def _combine_close(got, planes, coefs, what):
    ref, S = E.combine_ref(planes, coefs)
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    bnd = E.combine_bound(len(coefs), S, planes.dtype)
    ratio = float((err / bnd).max())
    print("%s: max |got - ref| / (K eps S) = %.3f" % (what, ratio))
    assert (err <= bnd).all(), "%s: %d elements beyond K eps S, worst ratio %.3g" % (what, (err > bnd).sum(), ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_combine_planes_within_the_derived_bound_and_exact_where_products_are(torch_cuda, dtype):
    """K = 1 to 8.  Random coefficients in [-3, 3], planes over six decades: |got - ref| <= K eps S.  Coefficients +-2^j (K = 2:
    the gdd pair [1, -1]): the bits of the typed left-to-right sum, which a fused multiply-add leaves as they are."""
    from climate_toolbox_amd import engine
    for K in range(1, 9):
        planes, coefs = E.combine_random_case(dtype, K, 257, 100 + K)
        got = _host(engine.combine_planes(_dev(torch_cuda, planes), coefs))
        assert got.dtype == dtype and got.shape == (257,)
        _combine_close(got, planes, coefs, "K=%d" % K)
        planes, coefs = E.combine_exact_case(dtype, K, 257, 200 + K)
        got = engine.combine_planes(_dev(torch_cuda, planes.reshape(K, 1, 257)), coefs)
        _same_bits(got, E.combine_typed(planes, coefs).reshape(1, 257), "exact K=%d %r" % (K, list(coefs)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_combine_planes_specials(torch_cuda, dtype):
    """a NaN plane gives NaN, 0 x inf gives NaN, inf - inf gives NaN, inf stays inf: the pattern of NumPy's typed sum"""
    from climate_toolbox_amd import engine
    planes = np.ones((3, 8), dtype)
    planes[0, 0] = np.nan
    planes[1, 1] = np.inf                                                   # times 0
    planes[0, 2], planes[2, 2] = np.inf, np.inf                             # 1 * inf + (-1) * inf
    planes[0, 3] = np.inf
    planes[2, 4] = -np.inf                                                  # (-1) * -inf
    planes[1, 5] = np.nan                                                   # 0 * NaN
    coefs = [1.0, 0.0, -1.0]
    want = E.combine_typed(planes, coefs)
    got = _host(engine.combine_planes(_dev(torch_cuda, planes), coefs))
    assert np.isnan(want[[0, 1, 2, 5]]).all() and want[3] == np.inf and want[4] == np.inf and (want[6:] == 0).all()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_combine_planes_plane_stride_and_refusals(torch_cuda, dtype):
    """through the C-ABI: plane_stride > n with NaN between the planes; plane_stride < n is refused for K > 1 (and ignored for
    one plane); K = 0 and K = 9 are refused"""
    from climate_toolbox_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    fn = L.wagg_combine_planes_f32 if dtype == np.float32 else L.wagg_combine_planes_f64
    K, n, ps = 3, 130, 141
    planes, coefs = E.combine_exact_case(dtype, K, n, 5)
    buf = np.full((K, ps), np.nan, dtype)
    buf[:, :n] = planes
    bd = _dev(torch, buf)
    out = torch.full((n + 4,), -7.5, dtype=bd.dtype, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(k, pstride, cf):
        cf = np.ascontiguousarray(cf, np.float64)
        return fn(C.c_void_p(bd.data_ptr()), k, pstride, cf.ctypes.data_as(C.POINTER(C.c_double)), n, C.c_void_p(out.data_ptr()), stream)

    _lib.check(call(K, ps, coefs), "wagg_combine_planes")
    got = _host(out)
    _same_bits(got[:n].copy(), E.combine_typed(planes, coefs), "plane_stride > n")
    assert (got[n:] == -7.5).all()
    _lib.check(call(1, 0, coefs[:1]), "wagg_combine_planes")
    _same_bits(_host(out)[:n].copy(), E.combine_typed(planes[:1], coefs[:1]), "one plane")
    with pytest.raises(_lib.WaggError, match="overlapping planes"):
        _lib.check(call(2, n - 1, coefs[:2]), "wagg_combine_planes")
    for k in (0, 9):
        with pytest.raises(_lib.WaggError, match="bad arguments"):
            _lib.check(call(k, ps, np.ones(9)), "wagg_combine_planes")


def test_combine_planes_second_trip(torch_cuda):
    """fp64, 524,288 + 77 elements per plane for 524,288 threads; fp32 likewise"""
    from climate_toolbox_amd import engine
    n = E.GRID_NARROW + 77
    for dtype, K in ((np.float64, 3), (np.float32, 2)):
        planes, coefs = E.combine_random_case(dtype, K, n, 300)
        _combine_close(_host(engine.combine_planes(_dev(torch_cuda, planes), coefs)), planes, coefs, "second trip %s" % dtype.__name__)
        planes, coefs = E.combine_exact_case(dtype, K, n, 301)
        _same_bits(engine.combine_planes(_dev(torch_cuda, planes), coefs), E.combine_typed(planes, coefs), "second trip, exact")


# ---- engine.transform_poly (xform_poly_kernel) -------------------------------------------------------------------------------------
def _poly_check(got, x, off, p, what):
    """bit-equal to the chain in the element type.  Underflow rule: an element whose IEEE result lies below the smallest
    normal must be that value or a zero of the same sign.  Returns how many such elements came back flushed."""
    want = E.poly_chain(x, off, p)
    tiny = np.finfo(x.dtype).tiny
    with np.errstate(invalid="ignore"):
        sub = np.abs(want) < tiny
    same = (E.bits(got) == E.bits(want)) | (np.isnan(got) & np.isnan(want))
    flushed = sub & ~same & (got == 0) & (np.signbit(got) == np.signbit(want))
    bad = ~same & ~flushed
    assert not bad.any(), "%s p=%d: %d differ, first x=%r got %r want %r" % (what, p, bad.sum(), x[bad][0], got[bad][0], want[bad][0])
    return int(flushed.sum()), int((sub & (want != 0)).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_transform_poly_is_the_typed_chain(torch_cuda, dtype):
    """powers 1 to 16 on Kelvin values with offset -273.15 and on values around 0 with offset 0; NaN; +-inf (-inf gives -inf
    at odd powers); values whose high powers overflow; values whose high powers pass through the subnormals to 0.  The MI355X
    gives the IEEE subnormal in both types: no element came back flushed to zero (the count is printed)."""
    from climate_toolbox_amd import _lib, engine
    flushed = subnormal = 0
    for kelvin, off in ((True, -273.15), (False, 0.0)):
        x = E.poly_values(dtype, kelvin)
        xd = _dev(torch_cuda, x)
        for p in range(1, 17):
            got = _host(engine.transform_poly(xd, off, p))
            f, s = _poly_check(got, x, off, p, "kelvin" if kelvin else "plain")
            flushed, subnormal = flushed + f, subnormal + s
            ninf = x == -np.inf
            assert ninf.any() and (got[ninf] == (-np.inf if p % 2 else np.inf)).all() and np.isnan(got[np.isnan(x)]).all()
        assert np.isinf(got[np.isfinite(x)]).any(), "a finite value overflows at power 16"
    print("transform_poly %s: %d subnormal results, %d of them flushed to zero" % (dtype.__name__, subnormal, flushed))
    assert subnormal > 10
    for p in (0, 17, -1):
        with pytest.raises(_lib.WaggError, match="bad arguments"):
            engine.transform_poly(xd, 0.0, p)
    x2 = E.poly_values(dtype, False)[:60].reshape(6, 10)
    got = _host(engine.transform_poly(_dev(torch_cuda, x2)[::2, 1::3], 1.5, 3))
    _poly_check(got, np.ascontiguousarray(x2[::2, 1::3]), 1.5, 3, "stepped view")


def test_transform_poly_second_trip(torch_cuda):
    from climate_toolbox_amd import engine
    for dtype in DTYPES:
        x = np.resize(E.poly_values(dtype, True), E.GRID_NARROW + 33)
        got = _host(engine.transform_poly(_dev(torch_cuda, x), -273.15, 3))
        assert got.size > E.GRID_NARROW
        _poly_check(got, x, -273.15, 3, "second trip")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_poly_apply_evaluates_the_same_device_function(torch_cuda, dtype):
    """csrc/wagg_util.hip: "the same device functions the aggregation kernels evaluate on load".  A segment table in which
    region r holds exactly one cell with weight 1.0 (a permutation of the grid): the fused poly apply, powers 1 to 4, also
    begun at power 2, equals transform_poly at those cells bit for bit (x * 1.0 / 1.0 is x)."""
    from climate_toolbox_amd import engine
    nlat, nlon, T = 12, 80, 70
    G = nlat * nlon
    rng = np.random.default_rng(11)
    code = rng.permutation(G).astype(np.int32)
    X = (288.0 + 15.0 * rng.standard_normal((T, G))).astype(dtype)
    Xd = _dev(torch_cuda, X)
    plan = engine.SparsePlan(np.arange(G, dtype=np.int32), code, np.ones(G), G, G, row_len=nlon)
    try:
        for layout, xin in (("TG", Xd), ("GT", _dev(torch_cuda, X.T))):
            got = _host(plan.apply_poly(xin, -273.15, 4, layout=layout))
            for p in range(1, 5):
                want = _host(engine.transform_poly(Xd, -273.15, p))
                _same_bits(np.ascontiguousarray(got[p - 1][:, code]), want, "fused power %d %s" % (p, layout))
                _same_bits(want, E.poly_chain(X, -273.15, p), "transform_poly power %d" % p)
        got = _host(plan.apply_poly(Xd, -273.15, 2, pow_first=2))
        for k, p in enumerate((2, 3)):
            _same_bits(np.ascontiguousarray(got[k][:, code]), E.poly_chain(X, -273.15, p), "pow_first 2, power %d" % p)
        plan.status()
    finally:
        plan.close()


# ---- engine.transform_edd (xform_edd_kernel): the second trip and the refusal only ---------------------------------------------------
def test_transform_edd_second_trip_with_eight_terms(torch_cuda):
    """fp64, 513 x 1024 = 525,312 elements for 524,288 threads, 8 terms: against the expectation of tests/test_gpu_edd_edges.py
    term by term -- every term's own bound times |c_k| (in band the module's bound; where the reference selects, the distance
    of the typed value that module demands bit for bit from the high-precision one), plus K eps sum_k |c_k ref_k| for the K products and K - 1 sums
    (the bound of combine_planes).  9 terms are refused."""
    from climate_toolbox_amd import _lib, engine
    from tests import edd_edges as EE
    from tests import test_gpu_edd_edges as GE
    dtype, grid, T = np.float64, (16, 64), 513
    lo, hi = GE._fields.__wrapped__(dtype, False, "all", grid, T, False)
    assert lo.size > E.GRID_NARROW
    coefs = [1.0, -1.0, 0.5, 2.0, -0.75, 1.25, -3.0, 0.3]
    thr = list(EE.THRESHOLDS) + [12.5, 20.0, 25.5]
    lod, hid = _dev(torch_cuda, lo.copy()), _dev(torch_cuda, hi.copy())
    got = _host(engine.transform_edd(lod, hid, 0.0, list(zip(coefs, thr)))).reshape(lo.shape)
    ref, bnd, scale = np.zeros(lo.shape, np.longdouble), np.zeros(lo.shape), np.zeros(lo.shape)
    nan = np.zeros(lo.shape, bool)
    for c, e in zip(coefs, thr):
        x = GE._expect.__wrapped__(dtype, False, "all", grid, T, False, e)
        with np.errstate(invalid="ignore"):
            ref += np.longdouble(c) * x.ref
        nan |= ~np.isfinite(x.ref)
        bk = np.zeros(lo.shape)
        bk[x.band] = EE.bound(x.ylo[x.band], x.yhi[x.band], e, dtype, "libm")
        sel = x.outer & np.isfinite(x.ref)                      # selected elements are (y_max + y_min) / 2 - e in the type, bit
        bk[sel] = np.abs(x.vals[sel] - x.ref[sel]).astype(np.float64)   # for bit in that module: their distance from the reference
        bnd += abs(c) * bk
        scale += abs(c) * np.abs(np.where(np.isfinite(x.ref), x.ref, 0)).astype(np.float64)
    bnd += len(coefs) * E.eps(dtype) * scale
    fin = ~nan
    assert fin.sum() > E.GRID_NARROW // 2 and np.isfinite(got[fin]).all()
    err = np.abs(got[fin].astype(np.longdouble) - ref[fin]).astype(np.float64)
    worst = float((err / np.maximum(bnd[fin], 1e-300)).max())
    print("transform_edd, 8 terms, second trip: max error / bound = %.3f" % worst)
    assert (err <= bnd[fin]).all(), worst
    tail = slice(E.GRID_NARROW // grid[0] // grid[1] * grid[0] * grid[1], None)
    assert fin.ravel()[tail].any()                                          # (elements of the second trip are among those compared)
    with pytest.raises(_lib.WaggError, match="bad arguments"):
        engine.transform_edd(lod, hid, 0.0, [(1.0, 8.0)] * 9)


# ---- the drop-in on device-resident fields -------------------------------------------------------------------------------------------
DIM_ORDERS = [("time", "lat", "lon"), ("lat", "lon", "time"), ("lat", "time", "lon"), ("member", "time", "lat", "lon"),
              ("lat", "lon", "member", "time"), ("time", "lon", "lat"), ("lon", "member", "lat"), ("lat", "lon")]
SIZES = {"time": 9, "member": 3, "lat": 12, "lon": 17}


@pytest.mark.parametrize("dims", DIM_ORDERS, ids=["-".join(d) for d in DIM_ORDERS])
def test_dropin_on_device_fields_equals_the_host_call_in_every_dim_order(torch_cuda, dims):
    """The eight dim orders and the segment table of test_dropin_any_dim_order_and_label_types (string labels with nulls, NaN
    weights): weighted_aggregate_grid_to_regions on a CUDA tensor of float32, float64, int16 and float16 data equals the same
    call on the host array of the same numbers bit for bit.  Both routes hand the same (T x G) / (G x T) matrix to the same
    cached plan: the host route through the row-block pipeline (one block here) or an upload, the device route through
    relayout / to_float64 -- the kernels of the apply are the same."""
    from climate_toolbox_amd import minixr, weighted_aggregate_grid_to_regions
    torch = torch_cuda
    rng = np.random.default_rng(len(dims) * 7 + len(dims[0]))
    lat, lon = np.linspace(-55, 55, SIZES["lat"]), np.linspace(-160, 170, SIZES["lon"])
    shape = [SIZES[d] for d in dims]
    whole = rng.integers(250, 311, shape)                                   # exact in every type, float16 included
    coords = {d: (lat if d == "lat" else lon if d == "lon" else np.arange(SIZES[d])) for d in dims}
    n = 400
    labels = np.array(["R%02d" % k for k in rng.integers(0, 25, n)], dtype=object)
    labels[rng.random(n) < 0.05] = None
    df = pd.DataFrame({"lat": rng.choice(lat, n), "lon": rng.choice(lon, n), "areawt": rng.uniform(0.1, 1, n),
                       "popwt": np.where(rng.random(n) < 0.2, np.nan, rng.uniform(0, 4, n)), "hierid": labels})
    nans = rng.integers(0, whole.size, 3)
    for dt in (np.float32, np.float64, np.int16, np.float16):
        vals = whole.astype(dt)
        if vals.dtype.kind == "f":
            vals.flat[nans] = np.nan
        outs = []
        for wrap in (lambda v: v, lambda v: torch.from_numpy(v.copy()).cuda()):
            ds = minixr.Dataset({"tas": (dims, wrap(vals))}, coords=coords)
            out = weighted_aggregate_grid_to_regions(ds, "tas", "popwt", "hierid", df)
            outs.append(np.asarray(out.tas.values))
        assert np.isfinite(outs[0]).sum() > outs[0].size // 2
        _same_bits(outs[1], outs[0], "%s %s" % (dims, np.dtype(dt).name))


@pytest.mark.parametrize("nlon", [16, 17])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_standardize_on_device_fields_equals_the_host_call(torch_cuda, dtype, nlon):
    """a 29 February and a 0..360 longitude axis on device tensors with lon last and with lon not last: the standardised,
    leap-day-free field (take_axis along lon and along time; nlon = 16 gives rows of whole 16-byte pieces, 17 does not) and
    its aggregate equal the host call's bit for bit"""
    from climate_toolbox_amd import minixr, standardize_climate_data, weighted_aggregate_grid_to_regions
    from climate_toolbox_amd.transformations import remove_leap_days
    torch = torch_cuda
    rng = np.random.default_rng(nlon)
    nlat = 6
    lat, lon360 = np.linspace(-25, 25, nlat), np.arange(nlon) * (360.0 / nlon)
    lon180 = np.sort((lon360 + 180) % 360 - 180)
    time = pd.date_range("2004-02-20", periods=20).values
    tas = (280 + 8 * rng.standard_normal((len(time), nlat, nlon))).astype(dtype)
    tas.flat[rng.integers(0, tas.size, 4)] = np.nan
    n = 150
    df = pd.DataFrame({"lat": rng.choice(lat, n), "lon": rng.choice(lon180, n), "areawt": rng.uniform(0.1, 1, n), "hierid": rng.integers(0, 12, n)})
    for dims, order in ((("time", "lat", "lon"), (0, 1, 2)), (("lon", "time", "lat"), (2, 0, 1)), (("time", "lon", "lat"), (0, 2, 1))):
        vals = np.ascontiguousarray(tas.transpose(order))
        fields, outs = [], []
        for wrap in (lambda v: v, lambda v: torch.from_numpy(v.copy()).cuda()):
            ds = minixr.Dataset({"tas": (dims, wrap(vals))}, coords={"time": time, "lat": lat, "lon": lon360})
            ds = remove_leap_days(standardize_climate_data(ds))
            np.testing.assert_array_equal(ds.coords["lon"].values, lon180)
            fields.append(np.asarray(ds["tas"].values))
            outs.append(np.asarray(weighted_aggregate_grid_to_regions(ds, "tas", "areawt", "hierid", df).tas.values))
        assert fields[0].shape[dims.index("time")] == 19 and fields[0].shape[dims.index("lon")] == nlon
        _same_bits(fields[1], fields[0], "standardised field %s" % (dims,))
        # (and the host field is what NumPy makes of the raw array: the leap day gone, the columns in -180..180 order)
        perm = np.argsort((lon360 + 180) % 360 - 180, kind="stable")
        keep = np.flatnonzero(time != np.datetime64("2004-02-29"))
        _same_bits(fields[0], np.take(np.take(vals, keep, axis=dims.index("time")), perm, axis=dims.index("lon")), "host field %s" % (dims,))
        _same_bits(outs[1], outs[0], "aggregate %s" % (dims,))


# ---- the random driver ---------------------------------------------------------------------------------------------------------------
FUZZ_ELEMENTS_CASES, FUZZ_ELEMENTS_SEED = 36, 2031


def test_randomised_element_cases(torch_cuda):
    """tests/fuzz_gpu.py's elements_case (FUZZ_ELEMENTS=1), 36 seeded cases: a kernel of relayout / to_float64 / take_axis /
    gather, a dtype, 1 to 6 dims of extents 1 to 9, steps, an order, an index list; bits against tests/element_ops.py"""
    from tests.test_gpu_dense_forms_small import _fuzz_module
    fz = _fuzz_module()
    rng = np.random.default_rng(FUZZ_ELEMENTS_SEED)
    failures, tags = [], []
    for i in range(FUZZ_ELEMENTS_CASES):
        tag, fails = fz.elements_case(i, rng)
        tags.append(tag)
        assert fails is not None, "every case is compared"
        if fails:
            failures.append(tag + " | " + "; ".join(fails))
    assert not failures, "\n".join(failures)
    n = {k: sum("[kernel %s]" % k in tag for tag in tags) for k in ("relayout", "to_float64", "take_axis", "gather")}
    print("element cases:", n)
    assert min(n.values()) >= 4, n
