"""Restatements and case builders for the element and data-movement kernels of csrc/wagg_util.hip (gather, xform_poly,
any_less, combine_planes, take_axis, relayout, relayout_to_f64), shared by tests/test_element_ops_host.py (no GPU),
tests/test_gpu_element_ops.py and the FUZZ_ELEMENTS leg of tests/fuzz_gpu.py.  NumPy only; torch is not imported here.

Data movement is compared as INTEGER BIT PATTERNS (:func:`bits`), so NaN payloads and -0.0 count.  The address rule of
relayout / to_float64 is :func:`walk`; the conversions to fp64 are written from the formats' definitions, not with
NumPy's casts, where that is possible (:func:`to_f64_ref`); the polynomial is the multiplication chain in the element
type (:func:`poly_chain`); combine_planes has a high-precision value with its scale (:func:`combine_ref`), the typed
left-to-right sum (:func:`combine_typed`) and the same sum with every ``s + c * p`` rounded once (:func:`combine_fused`).

The bound of combine_planes is derived, not measured: K products and K - 1 sums, each with a relative error of at most
u = eps / 2 of a magnitude of at most S = sum_k |c_k| |p_k| (to first order), so |got - ref| <= (2K - 1) u S < K eps S --
whether or not a product and its sum are contracted into one fused multiply-add, which only removes roundings."""
import collections
import fractions
import math

import numpy as np

GRID_WIDE = 4096 * 256            # threads of take_axis / relayout / relayout_to_f64: one trip covers this many elements
GRID_NARROW = 2048 * 256          # threads of xform_poly / xform_edd / any_less / combine_planes
BIG2D = (1031, 1019)              # 1,050,589 elements: more than GRID_WIDE, both extents prime


def bits(a):
    """the array as unsigned integers of its element size"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def eps(dtype):
    return float(np.finfo(dtype).eps)


# ---- fills ---------------------------------------------------------------------------------------------------------------------------
_SPECIAL32 = (0x7fc00000, 0xffc00000, 0x7f800001, 0x7fc12345, 0xffffffff, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
              0x00000001, 0x807fffff, 0x00800000, 0x7f7fffff)
_SPECIAL64 = (0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0x7ff8000012345678, 0xffffffffffffffff,
              0x7ff0000000000000, 0xfff0000000000000, 0x8000000000000000, 0x0000000000000000, 0x0000000000000001,
              0x800fffffffffffff, 0x0010000000000000, 0x7fefffffffffffff)


def random_words(n, dtype, seed):
    """``n`` elements of ``dtype`` (float32 / float64) from random 32- / 64-bit words, with quiet and signalling NaNs of
    several payloads, +-inf, -0, +0, subnormals and the largest finite number planted at fixed and at random places"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        w, sp = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.array(_SPECIAL32, np.uint32)
    else:
        w, sp = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64), np.array(_SPECIAL64, np.uint64)
    k = min(n, len(sp))
    w[:k] = sp[:k]
    if n > 4 * len(sp):
        w[rng.integers(k, n, 2 * len(sp))] = np.tile(sp, 2)
    return w.view(dtype)


# ---- the address walk ------------------------------------------------------------------------------------------------------------------
def walk(shape, strides):
    """Source offset (in elements) of every destination element, in destination order: the mixed-radix digits of the
    destination index, last dim fastest, each times its stride"""
    total = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    rem = np.arange(total, dtype=np.int64)
    off = np.zeros(total, dtype=np.int64)
    for k in range(len(shape) - 1, -1, -1):
        if total:
            off += (rem % shape[k]) * strides[k]
            rem = rem // shape[k]
    return off


View = collections.namedtuple("View", "name nbuf base shape strides order")
"""a strided view of a flat buffer of ``nbuf`` elements: it begins at element ``base`` and has ``shape`` / ``strides`` (in
elements); ``order`` is the permutation asked of relayout / to_float64"""


def view_of(buf, v):
    """the NumPy view ``v`` describes, over the flat array ``buf``"""
    it = buf.dtype.itemsize
    return np.lib.stride_tricks.as_strided(buf[v.base:], shape=v.shape, strides=[s * it for s in v.strides], writeable=False)


def relayout_ref(buf, v):
    """what relayout(view, order) holds: the walk over the permuted shape and strides"""
    shape, strides = [v.shape[i] for i in v.order], [v.strides[i] for i in v.order]
    return buf[v.base + walk(shape, strides)].reshape(shape)


def _describe(name, flat, view, order):
    """View record of a NumPy view made by slicing / broadcasting ``flat`` (so that walk is checked against NumPy's own
    strides, not against as_strided)"""
    it = flat.dtype.itemsize
    base = (view.__array_interface__["data"][0] - flat.__array_interface__["data"][0]) // it
    assert all(s % it == 0 and s >= 0 for s in view.strides)
    return View(name, flat.size, int(base), tuple(int(s) for s in view.shape), tuple(int(s) // it for s in view.strides), tuple(order))


SHAPES = {1: (13,), 2: (5, 7), 3: (3, 5, 4), 4: (3, 4, 2, 5), 5: (2, 3, 2, 3, 2), 6: (2, 3, 2, 1, 3, 2)}


def orders(nd):
    """identity, full reversal, a swap of non-adjacent dims, and (3, 1, 0, 2) where there are four"""
    out = [tuple(range(nd))]
    if nd >= 2:
        out.append(tuple(range(nd - 1, -1, -1)))
    if nd >= 3:
        sw = list(range(nd))
        sw[0], sw[nd - 1] = sw[nd - 1], sw[0]
        out.append(tuple(sw))
    if nd == 4:
        out.append((3, 1, 0, 2))
    return out


def source_views(nd):
    """[(name, flat array of int64 positions, view)]: contiguous; sliced with a step (and so beginning inside the buffer);
    beginning one element into the buffer; an expanded dim (stride 0); dims of extent 1"""
    shape = SHAPES[nd]
    n = int(np.prod(shape))
    out = []
    flat = np.arange(n, dtype=np.int64)
    out.append(("contiguous", flat, flat.reshape(shape)))
    big = tuple(2 * s + 1 for s in shape)
    flat = np.arange(int(np.prod(big)), dtype=np.int64)
    out.append(("stepped", flat, flat.reshape(big)[tuple(slice(1 - k % 2, 2 * s + 1 - k % 2, 2) for k, s in enumerate(shape))]))
    flat = np.arange(n + 1, dtype=np.int64)
    out.append(("offset base", flat, flat[1:].reshape(shape)))
    one = list(shape)
    one[nd // 2] = 1
    flat = np.arange(int(np.prod(one)), dtype=np.int64)
    out.append(("expanded", flat, np.broadcast_to(flat.reshape(one), shape)))
    ones = list(shape)
    ones[0] = ones[-1] = 1
    flat = np.arange(2 * int(np.prod(ones)), dtype=np.int64)
    out.append(("extent 1", flat, flat[::2].reshape(ones)))
    return out


def relayout_views():
    """every View of the small relayout / to_float64 cases: 1 to 6 dims x five sources x the orders"""
    out = []
    for nd in range(1, 7):
        for name, flat, view in source_views(nd):
            assert view.shape == tuple(SHAPES[nd]) or name == "extent 1"
            for order in orders(nd):
                out.append((_describe("%dd %s %r" % (nd, name, order), flat, view, order), flat, view))
    flat = np.arange(3 * 5 * 4, dtype=np.int64)
    empty = flat.reshape(3, 5, 4)[:, 2:2, :]
    out.append((_describe("extent 0", flat, empty, (2, 0, 1)), flat, empty))
    return out


def big_view():
    """BIG2D transposed: one element more trips than GRID_WIDE threads cover"""
    n = BIG2D[0] * BIG2D[1]
    return View("second trip", n, 0, BIG2D, (BIG2D[1], 1), (1, 0))


def stepped3d(nbuf=256):
    """a stepped, permuted 3-D view of a 4 x 8 x 8 buffer (every type of to_float64 runs through it once)"""
    assert nbuf == 256
    flat = np.arange(nbuf, dtype=np.int64)
    view = flat.reshape(4, 8, 8)[::2, 1:, ::3]
    return _describe("stepped 3-D", flat, view, (2, 0, 1))


# ---- conversions to fp64 ---------------------------------------------------------------------------------------------------------------
def bf16_to_f64(b):
    """bf16 bit patterns (uint16): the upper half of a float32, widened"""
    with np.errstate(invalid="ignore"):                            # (signalling NaNs among the patterns)
        return (np.asarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def f16_to_f64(b):
    """f16 bit patterns (uint16) decoded from sign, exponent and mantissa"""
    b = np.asarray(b, np.uint16).astype(np.int64)
    sign, e, m = b >> 15, (b >> 10) & 31, b & 1023
    mag = np.where(e == 0, np.ldexp(m.astype(np.float64), -24), np.ldexp((1024 + m).astype(np.float64), (e - 25).astype(np.int64)))
    mag = np.where(e == 31, np.where(m == 0, np.inf, np.nan), mag)
    return np.where(sign == 1, -mag, mag)


def int_to_f64(a):
    """Python's float(int): round to nearest, ties to even"""
    a = np.asarray(a)
    return np.array([float(int(v)) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


INT64_EDGES = (2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 + 1), 2 ** 63 - 1, -2 ** 63, 2 ** 53, 2 ** 53 - 1, 2 ** 62 + 2 ** 8 + 1, 0, 1, -1)

TO_F64_KINDS = ("float16", "bfloat16", "int8", "uint8", "int16", "int32", "int64", "float32", "float64")


def to_f64_values(kind, seed=5):
    """the source values of ``kind`` as a NumPy array (float16 / bfloat16: their uint16 bit patterns, all 65,536)"""
    rng = np.random.default_rng(seed)
    if kind in ("float16", "bfloat16"):
        return np.arange(65536, dtype=np.uint32).astype(np.uint16)
    if kind == "int16":
        return np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    if kind == "int8":
        return np.arange(-128, 128, dtype=np.int16).astype(np.int8)
    if kind == "uint8":
        return np.arange(256, dtype=np.int16).astype(np.uint8)
    if kind == "int32":
        return np.concatenate([np.array([-2 ** 31, 2 ** 31 - 1, 0, 1, -1, 2 ** 24 + 1, -(2 ** 24 + 1)], np.int64),
                               rng.integers(-2 ** 31, 2 ** 31, 505)]).astype(np.int32)
    if kind == "int64":
        return np.concatenate([np.array(INT64_EDGES, np.int64), rng.integers(-2 ** 63, 2 ** 63 - 1, 501, dtype=np.int64, endpoint=True)])
    return random_words(512, np.float32 if kind == "float32" else np.float64, seed)


def to_f64_ref(kind, values):
    """fp64 of ``values`` (as :func:`to_f64_values` gives them) by the restatement of ``kind``"""
    if kind == "float16":
        return f16_to_f64(values)
    if kind == "bfloat16":
        return bf16_to_f64(values)
    if kind == "float32":
        with np.errstate(invalid="ignore"):
            return np.asarray(values, np.float32).astype(np.float64)   # (exact: every float32 is a float64)
    if kind == "float64":
        return np.asarray(values, np.float64)
    return int_to_f64(values)


def same_f64(got, ref, exact_nan=False):
    """None, or what differs: non-NaN as bits, NaN as NaN (as bits too with ``exact_nan``)"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return "shape / dtype %r %s vs %r %s" % (got.shape, got.dtype, ref.shape, ref.dtype)
    gb, rb = bits(got).ravel(), bits(ref).ravel()
    ok = gb == rb
    if not exact_nan and got.dtype.kind == "f":
        ok |= np.isnan(got).ravel() & np.isnan(ref).ravel()
    if ok.all():
        return None
    i = int(np.flatnonzero(~ok)[0])
    return "%d of %d differ, first at %d: got %#x, want %#x" % ((~ok).sum(), ok.size, i, int(gb[i]), int(rb[i]))


# ---- the polynomial chain --------------------------------------------------------------------------------------------------------------
def poly_chain(x, off, p):
    """(x + off) ** p as the device evaluates it: y = x + T(off); r = y; r *= y, p - 1 times; every step in x's type"""
    T = x.dtype.type
    with np.errstate(all="ignore"):
        y = x + T(off)
        r = y
        for _ in range(p - 1):
            r = r * y
        assert y.dtype == x.dtype and r.dtype == x.dtype
    return r


def poly_values(dtype, kelvin):
    """Kelvin temperatures (for offset -273.15) or values around 0 (offset 0), then the specials: NaN, +-inf, values whose
    high powers overflow, values whose high powers underflow (through the subnormals to 0), +-0 and a subnormal"""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(17 + int(kelvin))
    fi = np.finfo(dtype)
    base = (288.0 + 15.0 * rng.standard_normal(300)) if kelvin else 30.0 * rng.standard_normal(300)
    shift = 273.15 if kelvin else 0.0
    big = float(fi.max) ** (1.0 / np.array([1.5, 2.5, 3.5, 7.5, 15.5]))            # overflow from power 2, 3, 4, 8, 16
    small = float(fi.tiny) ** (1.0 / np.array([1.5, 2.5, 3.5, 7.5, 15.5]))          # below the smallest normal likewise
    into = (float(fi.tiny) / 1024) ** (1.0 / np.array([2.0, 3.0, 4.0, 8.0, 16.0]))  # that power lands among the subnormals
    sub = float(fi.tiny) * float(fi.eps) * 37                                        # a subnormal: its square is 0
    special = np.concatenate([big, -big, small, -small, small * 0.9, -small * 1.1, into, -into,
                              [sub, -sub, float(fi.tiny), -float(fi.tiny)]]) + shift
    x = np.concatenate([base, special]).astype(dtype)
    x = np.concatenate([x, np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype)])
    return x


# ---- combine_planes --------------------------------------------------------------------------------------------------------------------
def _wide(dtype):
    if np.dtype(dtype) == np.float32:
        return np.float64
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is too short to carry the fp64 reference"
    return np.longdouble


def combine_ref(planes, coefs):
    """(value, S): sum_k c_k p_k with the coefficients rounded to the element type first, summed in higher precision
    (fp64 for fp32 planes, where every product is exact; np.longdouble for fp64 planes), and S = sum_k |c_k| |p_k| in fp64"""
    T, W = planes.dtype.type, _wide(planes.dtype)
    c = np.asarray(coefs, np.float64).astype(T)
    with np.errstate(all="ignore"):
        val = sum(W(c[k]) * planes[k].astype(W) for k in range(len(c)))
        S = sum(abs(float(c[k])) * np.abs(planes[k].astype(np.float64)) for k in range(len(c)))
    return val, S


def combine_typed(planes, coefs):
    """s = c0 * p0; s += ck * pk, left to right, every product and every sum rounded to the element type"""
    T = planes.dtype.type
    c = np.asarray(coefs, np.float64).astype(T)
    with np.errstate(all="ignore"):
        s = c[0] * planes[0]
        for k in range(1, len(c)):
            s = s + c[k] * planes[k]
    assert s.dtype == planes.dtype
    return s


def combine_fused(planes, coefs):
    """the same sum with every ``s + ck * pk`` rounded ONCE (a fused multiply-add): for fp32 planes computed in fp64 and
    rounded; for fp64 planes exactly, in rationals (finite planes only)"""
    T = planes.dtype.type
    c = np.asarray(coefs, np.float64).astype(T)
    with np.errstate(all="ignore"):
        s = c[0] * planes[0]
        for k in range(1, len(c)):
            if T is np.float32:
                s = (s.astype(np.float64) + np.float64(c[k]) * planes[k].astype(np.float64)).astype(np.float32)
            else:
                F = fractions.Fraction
                ck = F(float(c[k]))
                s = np.array([float(F(float(a)) + ck * F(float(b))) for a, b in zip(s, planes[k])], dtype=np.float64)
    return s


def combine_bound(K, S, dtype):
    return K * eps(dtype) * np.asarray(S, np.float64)


def combine_random_case(dtype, K, n, seed):
    """coefficients uniform in [-3, 3], planes of both signs spanning six decades (1e-3 .. 1e3)"""
    rng = np.random.default_rng(seed)
    coefs = rng.uniform(-3, 3, K)
    planes = (rng.choice([-1.0, 1.0], (K, n)) * 10.0 ** rng.uniform(-3, 3, (K, n))).astype(dtype)
    return planes, coefs


def combine_exact_case(dtype, K, n, seed):
    """coefficients +-2^j, j in -3 .. 3 (K = 2: the gdd pair [1, -1]); planes of both signs in 2^-6 .. 2^6: every product
    is exact, so the typed sum and the fused one are the same operations"""
    rng = np.random.default_rng(seed)
    coefs = rng.choice([-1.0, 1.0], K) * 2.0 ** rng.integers(-3, 4, K)
    if K == 2:
        coefs = np.array([1.0, -1.0])
    planes = (rng.choice([-1.0, 1.0], (K, n)) * 2.0 ** rng.uniform(-6, 6, (K, n))).astype(dtype)
    return planes, coefs


# ---- take_axis -------------------------------------------------------------------------------------------------------------------------
INNER_BYTES = (4, 8, 12, 16, 24, 48, 336)          # 16, 48, 336: the 16-byte kernel; the others the 4-byte one


def index_lists(n_src, seed=3):
    rng = np.random.default_rng(seed)
    return [("empty", np.zeros(0, np.int64)), ("one", np.array([n_src - 1])), ("reversed", np.arange(n_src)[::-1].copy()),
            ("repeated", np.array([0, 0, n_src - 1, 1 % n_src, 0, n_src - 1])), ("longer", rng.integers(0, n_src, 2 * n_src + 3))]


def take_shapes(dtype, inner_bytes, n_src=7):
    """[(shape, axis)] for one row size: axis first (outer 1), middle (outer 3), and their negative spellings; None when the
    element is larger than the row"""
    it = np.dtype(dtype).itemsize
    if inner_bytes % it:
        return []
    inner = inner_bytes // it
    out = [((n_src, inner), 0), ((3, n_src, inner), 1), ((3, n_src, inner), -2), ((n_src, inner), -2)]
    if inner > 1 and inner % 2 == 0:
        out.append(((3, n_src, inner // 2, 2), 1))                 # (the row spread over two trailing dims)
    return out


def take_big(dtype, wide):
    """(shape, axis, idx) whose destination is just more than GRID_WIDE 16-byte pieces (``wide``) or 4-byte words"""
    it = np.dtype(dtype).itemsize
    if wide:
        inner = 87382 * 16 // it                                   # 3 * 4 * 87,382 = 1,048,584 pieces
    else:
        inner = 87383 if it == 4 else 43691                        # 1,048,596 / 1,048,584 words; rows of 12 / 8 bytes mod 16
    assert (inner * it % 16 == 0) == wide and 3 * 4 * inner * it // (16 if wide else 4) > GRID_WIDE
    return (3, 3, inner), 1, np.array([2, 0, 2, 1])


# ---- gather ----------------------------------------------------------------------------------------------------------------------------
GATHER_T = (0, 1, 3, 70)
GATHER_NSEG = (0, 1, 255, 256, 257, 1000)


def gather_cells(G, nseg, seed):
    """``nseg`` cells of a grid of G with duplicates, the first cell and the last cell among them"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, G, nseg).astype(np.int32)
    if nseg >= 1:
        c[-1] = G - 1
    if nseg >= 2:
        c[0] = 0
    if nseg >= 4:
        c[2] = c[1]
    return c


def gather_ref(X_TG, cells, out_layout):
    """X_TG: the (T, G) matrix whatever the device layout is; the (T, nseg) or (nseg, T) result"""
    out = X_TG[:, cells]
    return out if out_layout == "TR" else np.ascontiguousarray(out.T)


# ---- any_less --------------------------------------------------------------------------------------------------------------------------
ANY_LESS_N = (1, 63, 64, 65, 256, GRID_NARROW + 1)


def any_less_pairs(dtype):
    """[(name, a, b, expected)] of single pairs decided by the comparison's own rules"""
    T = np.dtype(dtype).type
    return [("nan left", T(np.nan), T(1), False), ("nan right", T(0), T(np.nan), False), ("both nan", T(np.nan), T(np.nan), False),
            ("-0 < 0", T(-0.0), T(0.0), False), ("equal", T(3.25), T(3.25), False), ("-inf < inf", T(-np.inf), T(np.inf), True),
            ("inf < inf", T(np.inf), T(np.inf), False), ("one ulp", T(1), np.nextafter(T(1), T(2)), True),
            ("subnormal", T(0), T(np.finfo(T).tiny * np.finfo(T).eps), True), ("greater", T(2), T(1), False)]


def ref_any_less(a, b):
    with np.errstate(invalid="ignore"):
        return bool(np.any(a < b))


def fsum_rows(rows):
    """math.fsum down the first axis (exact, rounded once): used by the host test to check combine_ref's fp64 sums"""
    rows = np.asarray(rows, np.float64)
    return np.array([math.fsum(rows[:, i]) for i in range(rows.shape[1])])
