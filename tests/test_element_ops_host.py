"""The restatements of tests/element_ops.py checked without a GPU: the conversions against torch's and NumPy's casts over
every 16-bit pattern, the address walk against NumPy's own strided views, and the derived bound of combine_planes
(K eps S) against both emulations of the kernel's sum -- the typed left-to-right one and the one with every
``s + c * p`` rounded once -- so that the bound the GPU test asserts cannot hide a failure and does not count a fused
multiply-add as one."""
import numpy as np
import pytest

from tests import element_ops as E

DTYPES = [np.float32, np.float64]


def test_bf16_and_f16_restatements_equal_torch_and_numpy_over_all_patterns():
    import torch
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for kind, tdt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        mine = E.to_f64_ref(kind, b)
        theirs = [torch.from_numpy(b.view(np.int16).copy()).view(tdt).to(torch.float64).numpy()]
        if kind == "float16":
            theirs.append(b.view(np.float16).astype(np.float64))
        for t in theirs:
            assert E.same_f64(mine, t) is None, (kind, E.same_f64(mine, t))
            assert np.array_equal(np.isnan(mine), np.isnan(t))
        assert np.isnan(mine).sum() == (2046 if kind == "float16" else 254)
        assert np.signbit(mine[0x8000]) and mine[0x8000] == 0                       # -0 stays -0
    assert E.f16_to_f64(np.array([1], np.uint16))[0] == 2.0 ** -24 and E.bf16_to_f64(np.array([1], np.uint16))[0] == 2.0 ** -133


def test_integer_restatements_round_to_nearest_even():
    v = E.to_f64_values("int64")
    for must in (2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 + 1), 2 ** 63 - 1, -2 ** 63):
        assert must in [int(x) for x in v[:len(E.INT64_EDGES)]]
    ref = E.to_f64_ref("int64", v)
    assert E.same_f64(ref, v.astype(np.float64)) is None
    assert ref[0] == 2.0 ** 53 and ref[1] == 2.0 ** 53 + 4 and ref[2] == -2.0 ** 53 and ref[3] == 2.0 ** 63 and ref[4] == -2.0 ** 63
    for kind in ("int8", "uint8", "int16", "int32"):
        v = E.to_f64_values(kind)
        assert E.same_f64(E.to_f64_ref(kind, v), v.astype(np.float64)) is None
        assert len(np.unique(v)) == {"int8": 256, "uint8": 256, "int16": 65536}.get(kind, len(np.unique(v)))
    assert E.to_f64_values("int8").min() == -128 and E.to_f64_values("uint8").max() == 255


def test_random_words_hold_the_specials():
    for dt in DTYPES:
        x = E.random_words(4096, dt, 1)
        assert np.isnan(x).sum() >= 5 and np.isinf(x).sum() >= 2 and (np.signbit(x) & (x == 0)).any()
        tiny = np.finfo(dt).tiny
        assert ((np.abs(x) < tiny) & (x != 0)).any()
        assert len(np.unique(E.bits(x)[np.isnan(x)])) >= 4                           # several payloads


def test_walk_equals_numpy_on_every_builder_case():
    views = E.relayout_views()
    assert len(views) > 80
    names = " ".join(v.name for v, _, _ in views)
    for what in ("stepped", "offset base", "expanded", "extent 1", "extent 0", "(3, 1, 0, 2)"):
        assert what in names
    assert any(0 in v.strides for v, _, _ in views) and any(v.base == 1 for v, _, _ in views)
    for v, flat, view in views:
        want = np.ascontiguousarray(np.transpose(view, v.order))
        got = E.relayout_ref(flat, v)
        assert got.shape == want.shape and np.array_equal(got, want), v.name
        assert np.array_equal(E.view_of(flat, v), view), v.name
    v = E.stepped3d()
    flat = np.arange(256, dtype=np.int64)
    assert np.array_equal(E.relayout_ref(flat, v), np.ascontiguousarray(flat.reshape(4, 8, 8)[::2, 1:, ::3].transpose(2, 0, 1)))
    v = E.big_view()
    flat = np.arange(v.nbuf, dtype=np.int64)
    assert v.nbuf > E.GRID_WIDE and np.array_equal(E.relayout_ref(flat, v), np.ascontiguousarray(flat.reshape(E.BIG2D).T))


@pytest.mark.parametrize("dtype", DTYPES)
def test_poly_chain_is_the_typed_multiplication_chain(dtype):
    x = E.poly_values(dtype, kelvin=False)
    fi = np.finfo(dtype)
    r16, r2 = E.poly_chain(x, 0.0, 16), E.poly_chain(x, 0.0, 2)
    assert r16.dtype == dtype and np.isinf(r16).sum() > 10 and ((r16 == 0) & (x != 0)).sum() > 5
    assert ((np.abs(r2) < fi.tiny) & (r2 != 0)).any(), "a subnormal result is among the cases"
    ninf = x == -np.inf
    assert (E.poly_chain(x, 0.0, 3)[ninf] == -np.inf).all() and (r2[ninf] == np.inf).all()
    fin = np.isfinite(x) & (np.abs(x) < 100) & (np.abs(x) > 1e-3)
    np.testing.assert_allclose(E.poly_chain(x, 1.5, 5)[fin].astype(np.float64), (x[fin].astype(np.float64) + 1.5) ** 5, rtol=8 * fi.eps)
    k = E.poly_values(dtype, kelvin=True)
    assert np.array_equal(E.poly_chain(k, -273.15, 1), k + dtype(-273.15), equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_derived_bound_holds_for_both_emulations(dtype):
    """|emulation - ref| <= K eps S on every generated case, for the typed sum and for the once-rounded (fused) one; the
    largest share of the bound used is printed"""
    worst = 0.0
    for K in range(1, 9):
        for planes, coefs in (E.combine_random_case(dtype, K, 257, 100 + K), E.combine_exact_case(dtype, K, 257, 200 + K)):
            ref, S = E.combine_ref(planes, coefs)
            bnd = E.combine_bound(K, S, dtype)
            assert (S > 0).all()
            for emul in (E.combine_typed, E.combine_fused):
                got = emul(planes, coefs)
                err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
                assert (err <= bnd).all(), (K, emul.__name__, float((err / bnd).max()))
                worst = max(worst, float((err / bnd).max()))
    print("combine_planes emulations use at most %.3f of K eps S" % worst)
    assert worst < 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_coefficients_make_the_two_emulations_bit_equal(dtype):
    differ = 0
    for K in range(1, 9):
        planes, coefs = E.combine_exact_case(dtype, K, 257, 200 + K)
        m = np.abs(np.log2(np.abs(coefs)))
        assert (m == np.round(m)).all() and (K != 2 or list(coefs) == [1.0, -1.0])
        a, b = E.combine_typed(planes, coefs), E.combine_fused(planes, coefs)
        assert np.isfinite(a).all() and E.same_f64(a, b, exact_nan=True) is None, K
        # the products being exact, the correctly rounded sum of them (math.fsum) is what the reference must round to
        c = np.asarray(coefs).astype(dtype)
        exact = E.fsum_rows(np.stack([np.float64(c[k]) * planes[k].astype(np.float64) for k in range(K)]))
        ref, _ = E.combine_ref(planes, coefs)
        assert np.array_equal(ref.astype(np.float64), exact), K
        planes, coefs = E.combine_random_case(dtype, K, 257, 100 + K)
        differ += int((E.bits(E.combine_typed(planes, coefs)) != E.bits(E.combine_fused(planes, coefs))).sum())
    assert differ > 0, "with general coefficients the fused sum rounds differently somewhere: the emulations are two"


def test_case_builders_cover_what_the_gpu_module_names():
    assert set(E.INNER_BYTES) >= {4, 8, 12, 16, 48, 336}
    for dt in DTYPES:
        for wide in (True, False):
            shape, axis, idx = E.take_big(dt, wide)
            assert np.prod(shape[:axis]) * len(idx) * np.prod(shape[axis + 1:]) * np.dtype(dt).itemsize <= 18 << 20
        got = [ib for ib in E.INNER_BYTES if E.take_shapes(dt, ib)]
        assert got == ([4, 8, 12, 16, 24, 48, 336] if dt == np.float32 else [8, 16, 24, 48, 336])
    names = [n for n, _ in E.index_lists(7)]
    assert names == ["empty", "one", "reversed", "repeated", "longer"] and len(E.index_lists(7)[4][1]) > 7
    c = E.gather_cells(100, 257, 1)
    assert c[0] == 0 and c[-1] == 99 and c[1] == c[2] and c.dtype == np.int32
    assert E.GRID_NARROW + 1 in E.ANY_LESS_N
    for dt in DTYPES:
        for name, a, b, want in E.any_less_pairs(dt):
            assert E.ref_any_less(np.array([a]), np.array([b])) == want, name
