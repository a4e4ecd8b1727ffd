"""Snyder degree days element by element at the band edges: a generated catalogue of (tasmin, tasmax) pairs, a high-precision
reference of transformations.py:64-87 on the numbers the data type actually holds, the elements the reference SELECTS (compared
bit for bit) and a derived error bound for the elements inside the band.  No GPU and no torch: tests/test_edd_edges_host.py checks
this module, tests/test_gpu_edd_edges.py runs every degree-day kernel against it."""
import functools
from typing import NamedTuple

import numpy as np

try:
    import mpmath
except ImportError:                                             # the reference then runs in np.longdouble (asserted below)
    mpmath = None

THRESHOLDS = (-1.75, 8.0, 29.0, 30.3, 303.15)                   # (303.15: data left in Kelvin with offset 0)
CELSIUS_THRESHOLDS = THRESHOLDS[:4]
KELVIN = -273.15
ULPS = (0, 1, 2, 3, 16)
PARTNERS = (0.01, 0.1, 0.5, 1.0, 3.0, 7.3, 12.0, 25.0)
WIDTHS = (2.0 ** -20, 1.0, 12.0, 40.0)
ZS = (0.0, 0.5, 1 - 2.0 ** -10, 1 - 2.0 ** -20)
CLASSES = ("edge_x_edge", "tmin_edge_partner", "tmax_edge_partner", "tmin_above_edge", "tmax_below_edge", "above", "below",
           "flat_below", "flat_at", "flat_above", "inverted", "z_0", "z_0.5", "z_1-2^-10", "z_1-2^-20",
           "w_2^-20", "w_1", "w_12", "w_40", "nan_tmin", "nan_tmax_below", "nan_tmax_above", "nan_both")
INF_CLASSES = ("inf_tmax", "inf_tmin", "inf_both")
FIT = {"fit32": 5e-9, "fit64": 4.4e-15, "libm": 0.0}          # csrc/wagg_common.h, tools/fit_edd_poly.py
C_BOUND = {"fit32": 11.0, "fit64": 11.0, "libm": 12.0, "ieee": 8.0}


class Cases(NamedTuple):
    tasmin: np.ndarray
    tasmax: np.ndarray
    label: np.ndarray            # the class each pair was generated for (CLASSES, INF_CLASSES)
    inf: np.ndarray              # the separately flagged +-inf group


def steps(x, k, dtype):
    """``x`` moved ``k`` units in the last place of ``dtype`` (k < 0: down)"""
    x = dtype(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, dtype(np.inf if k > 0 else -np.inf), dtype=dtype)
    return x


def _generate(e, dtype, step):
    """(tasmin, tasmax, label) triples around the threshold ``e`` (already of ``dtype``); ``step(x, k)`` walks the grid the
    values live on (the type's own, or the coarser one raw Kelvin data lands on)"""
    f = dtype
    e64 = float(e)
    out = []

    def add(label, lo, hi):
        out.append((f(lo), f(hi), label))

    for k in ULPS:
        for m in ULPS:
            add("edge_x_edge", step(e, -k), step(e, m))
    for k in ULPS:
        for p in PARTNERS:
            add("tmin_edge_partner", step(e, -k), e64 + p)
            add("tmax_edge_partner", e64 - p, step(e, k))
    for k in ULPS:
        for p in PARTNERS[::2]:
            add("tmin_above_edge", step(e, k), e64 + p)           # tasmin >= e: the reference selects M - e
            add("tmax_below_edge", e64 - p, step(e, -k))          # tasmax <= e: the reference selects 0
    for a in (1e-3, 0.25, 4.0, 19.0):
        for b in (1e-3, 0.7, 9.0):
            add("above", e64 + a, e64 + a + b)
            add("below", e64 - a - b, e64 - a)
    for a in (13.0, 1.0, 1e-3):
        add("flat_below", e64 - a, f(e64 - a))
        add("flat_above", e64 + a, f(e64 + a))
    add("flat_at", e, e)
    add("flat_at", step(e, 1), step(e, 1))
    add("flat_at", step(e, -1), step(e, -1))
    for lo, hi in ((1.0, -5.0), (5.0, -1.0), (6.0, 2.0), (-2.0, -6.0), (0.0, -3.0), (3.0, 0.0), (1e-3, -1e-3)):
        add("inverted", e64 + lo, e64 + hi)                       # tasmin > tasmax
    znames = dict(zip(ZS, ("z_0", "z_0.5", "z_1-2^-10", "z_1-2^-20")))
    wnames = dict(zip(WIDTHS, ("w_2^-20", "w_1", "w_12", "w_40")))
    for w in WIDTHS:
        for z in ZS:
            for sign in ((1,) if z == 0 else (1, -1)):
                M = e64 - sign * z * w                            # z = (e - M) / w
                add(znames[z], M - w, M + w)
                add(wnames[w], M - w, M + w)
        for z in (0.1, -0.3, 0.77, -0.93):
            add(wnames[w], e64 - z * w - w, e64 - z * w + w)
    for a in (0.0, 1e-3, 2.0, 11.0):
        add("nan_tmin", np.nan, e64 + a)
        add("nan_tmin", np.nan, e64 - a)
        add("nan_tmax_below", step(e64 - a, -1 if a == 0 else 0), np.nan)     # tasmin < e: 0
        add("nan_tmax_above", e64 + a, np.nan)                                # tasmin >= e: M - e = NaN
        add("nan_both", np.nan, np.nan)
    inf = []
    for a in (-9.0, -1e-3, 0.0, 2.5):
        inf.append((f(e64 + a), f(np.inf), "inf_tmax"))           # tasmin < e: NaN (inf / inf); tasmin >= e: +inf
        inf.append((f(-np.inf), f(e64 + a), "inf_tmin"))          # tasmax > e: NaN; tasmax <= e: 0
    inf.append((f(-np.inf), f(np.inf), "inf_both"))
    inf.append((f(np.inf), f(np.inf), "inf_both"))
    inf.append((f(-np.inf), f(-np.inf), "inf_both"))
    return out, inf


def _cases(rows, inf_rows, dtype):
    lo = np.array([r[0] for r in rows + inf_rows], dtype=dtype)
    hi = np.array([r[1] for r in rows + inf_rows], dtype=dtype)
    label = np.array([r[2] for r in rows + inf_rows])
    inf = np.arange(len(lo)) >= len(rows)
    for a in (lo, hi, label, inf):
        a.setflags(write=False)
    return Cases(lo, hi, label, inf)


@functools.lru_cache(maxsize=None)
def catalogue(dtype, e):
    """The pairs around threshold ``e`` in ``dtype`` (np.float32 / np.float64), values the kernels see with ``offset = 0``"""
    rows, inf_rows = _generate(dtype(e), dtype, lambda x, k: steps(x, k, dtype))
    return _cases(rows, inf_rows, dtype)


def raw_for(y, offset, dtype):
    """The raw value ``x`` of ``dtype`` for which ``dtype(x + dtype(offset))`` lands nearest to ``y``"""
    off = dtype(offset)
    x = dtype(np.float64(y) - np.float64(off))
    if not np.isfinite(x):
        return x
    best = x
    for k in (-2, -1, 1, 2):
        c = steps(x, k, dtype)
        if abs(np.float64(dtype(c + off)) - np.float64(y)) < abs(np.float64(dtype(best + off)) - np.float64(y)):
            best = c
    return best


@functools.lru_cache(maxsize=None)
def catalogue_kelvin(dtype, e):
    """RAW pairs (Kelvin) for a degree-C threshold ``e``: ``dtype(x + dtype(-273.15))`` lands on the cases of
    :func:`catalogue`, with "k units in the last place" taken on the grid the shifted raw values live on (the spacing of the
    raw data near 273.15 + e, coarser than the type's own near e).  The type's own add is part of what is tested."""
    off = dtype(KELVIN)
    x_e = raw_for(dtype(e), KELVIN, dtype)
    e_land = dtype(x_e + off)                                     # == dtype(e) where 273.15 + e is on the raw grid

    def step(y, k):
        return dtype(steps(raw_for(y, KELVIN, dtype), k, dtype) + off)

    rows, inf_rows = _generate(e_land, dtype, step)
    raw = lambda v: raw_for(v, KELVIN, dtype) if np.isfinite(v) else v
    rows = [(raw(lo), raw(hi), lab) for lo, hi, lab in rows]
    inf_rows = [(raw(lo), raw(hi), lab) for lo, hi, lab in inf_rows]
    return _cases(rows, inf_rows, dtype)


def moved(x, offset, dtype):
    """the values exactly as the type moves them: ``dtype(x) + dtype(offset)`` in ``dtype``"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, dtype=dtype) + dtype(offset)).astype(dtype)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _band_hp(lo, hi, e):
    """transformations.py:65-72 for one in-band element (three exact binary numbers) in high precision, as np.longdouble"""
    if mpmath is not None:
        with mpmath.workprec(200):                              # 60 digits
            a, b, t = mpmath.mpf(float(lo)), mpmath.mpf(float(hi)), mpmath.mpf(float(e))
            M, w = (b + a) / 2, (b - a) / 2
            theta = mpmath.asin((t - M) / w)
            r = ((M - t) * (mpmath.pi / 2 - theta) + w * mpmath.cos(theta)) / mpmath.pi
            h = float(r)
            return np.longdouble(h) + np.longdouble(float(r - h))
    L = np.longdouble
    a, b, t = L(lo), L(hi), L(e)
    M, w = (b + a) / 2, (b - a) / 2
    theta = np.arcsin((t - M) / w)
    pi = L(np.pi) + L(1.2246467991473532e-16)
    return ((M - t) * (pi / 2 - theta) + w * np.cos(theta)) / pi


def reference(tasmin, tasmax, offset, e, dtype):
    """transformations.py:64-87 on the numbers the type holds -- ``y = dtype(x) + dtype(offset)`` in ``dtype``, ``dtype(e)``,
    the two selections on those rounded values (``y_min < e``, ``y_max > e``) -- evaluated in high precision (mpmath, 60
    digits; np.longdouble with a mantissa of at least 63 bits otherwise).  Returned as np.longdouble so that an fp64 result
    is not compared with a reference rounded to its own precision.  Non-finite inputs follow the formula in fp64 (NaN / inf
    patterns only)."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is too short to carry the reference"
    lo, hi, et = moved(tasmin, offset, dtype), moved(tasmax, offset, dtype), dtype(e)
    out = np.empty(lo.shape, dtype=np.longdouble)
    l64, h64, e64 = lo.astype(np.float64), hi.astype(np.float64), np.float64(et)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        M, w = (h64 + l64) / 2, (h64 - l64) / 2                   # (exact in fp64 for fp32 data; overwritten below in band)
        inner = np.where(h64 > e64, ((M - e64) * (np.pi / 2 - np.arcsin((e64 - M) / w)) + w * np.cos(np.arcsin((e64 - M) / w))) / np.pi, 0.0)
        out[...] = np.where(l64 < e64, inner, M - e64)
    band = (lo < et) & (hi > et) & np.isfinite(lo) & np.isfinite(hi)
    sel = ~(lo < et) & np.isfinite(lo) & np.isfinite(hi)          # M - e exactly (the sum of two fp64 numbers in longdouble
    L = np.longdouble                                             #  is exact up to one rounding at 2^-64)
    out[sel] = (L(1) * h64[sel] + L(1) * l64[sel]) / 2 - L(e64)
    for i in zip(*np.nonzero(band)):
        out[i] = _band_hp(lo[i], hi[i], et)
    return out


def in_band(tasmin, tasmax, offset, e, dtype):
    lo, hi, et = moved(tasmin, offset, dtype), moved(tasmax, offset, dtype), dtype(e)
    with np.errstate(invalid="ignore"):
        return (lo < et) & (hi > et) & np.isfinite(lo) & np.isfinite(hi)


def exact_outer(tasmin, tasmax, offset, e, dtype):
    """``(mask, values)``: the finite elements where the reference SELECTS -- ``!(y_min < e)``: ``M - e``; ``y_min < e`` and
    ``!(y_max > e)``: 0 -- and their values computed in ``dtype`` (``(y_max + y_min) / 2 - e`` and 0): the IEEE operations the
    device performs (``0.5 * s`` is exact, so contracting ``0.5 * s - e`` into an fma changes no bit).  Compared bit for bit,
    -0 and +0 both accepted where the value is 0."""
    lo, hi, et = moved(tasmin, offset, dtype), moved(tasmax, offset, dtype), dtype(e)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(lo) & np.isfinite(hi)
        first = ~(lo < et) & fin
        second = (lo < et) & ~(hi > et) & fin
        vals = np.where(first, ((hi + lo) / dtype(2) - et).astype(dtype), dtype(0)).astype(dtype)
    return first | second, vals


def bound(y_min, y_max, e, dtype, form):
    """Error bound of one in-band element, ``c u max(|y_min|, |y_max|, |e|, w) + fit w`` (u = 2^-24 / 2^-53: the unit roundoff).

    Derivation.  Exact inputs y_min < e < y_max; M = (y_max + y_min) / 2, w = (y_max - y_min) / 2, d = M - e, z = -d / w in
    (-1, 1), the value R = w f(z) with f(z) = (sqrt(1 - z^2) - z acos z) / pi, 0 <= f <= 1 + |z|, f(|z|) <= 1 / pi.  The partial
    derivatives: dR/dz = w f'(z) = -w acos(z) / pi, so |dR/dz| <= w; dR/dd (through z AND the closing max(d, 0) together: it
    is the true derivative of R) = acos(z) / pi, so |dR/dd| <= 1; dR/dw = sqrt(1 - z^2) / pi <= 1 / pi.  With S = max(|y_min|,
    |y_max|, |e|, w), and |d| < w <= S in band, operation by operation (each to first order in u):
      1. s = fl(y_max + y_min), M = s / 2 exact:          |dM| <= u |M| <= u S          -> through d:  1 u S
      2. d = fl(M - e):                                   u |d| <= u w                  -> through d:  1 u S
      3. w = fl(y_max - y_min) / 2:                       u w, times 1 / pi             ->          0.32 u S
      4. z = fl(d / w), correctly rounded division:       u |z|, times w                ->             1 u S
      5. t = fl(1 - |z|):                                 1.5 u on t^(3/2), times w / pi ->          0.48 u S
      6. sqrt(t), correctly rounded:                      u on the square root, times w / pi ->      0.32 u S
      7. Horner steps of P: each fma rounds once, the errors sum to <= u sum_k |p_k| <= 0.42 u (the partial sums of the
         coefficients), 1.4 u relative to P >= 0.30; the products sqrt(t) * t and (.) * P round once each
                                                          (1.4 + 2) u, times w / pi     ->          1.09 u S
      8. the closing fma fl(w q p + max(d, 0)):           u R <= u w                    ->             1 u S
    Sum 6.2 u S; counting every listed term as a whole u S gives c = 8 ("ieee": every operation correctly rounded).  The
    device's cheap forms replace the division by v_rcp_f32 (1 unit in the last place = 2 u) and a product (u): 3 u |z| against
    1 u |z|, + 2; fp64 takes v_rcp_f64 plus a Newton step (~2^-52 = 2 u) and a product, the same + 2.  v_sqrt_f32 (1 unit in the
    last place) and the fp64 v_rsq_f64 + Newton step add one more u on the square root: + 0.32, counted as + 1.  c = 11 for
    "fit32" and "fit64", plus the fit's own error |P_fit - P| <= fit (5e-9 / 4.4e-15) times w t^(3/2) <= w.
    The libm form ("libm", fp64 outside the loader/consumer kernel's finite items: ((M - e)(pi/2 - theta) + w c) / pi with
    theta = asin z, c = sqrt((1 - z)(1 + z))): terms 1-4 as above (4.32); asin within 2 units in the last place of
    |theta| <= pi / 2 (4 u pi / 2), times |d| / pi: 2; the rounding of pi / 2 - theta (<= u pi) times |d| / pi: 1; (1 - z),
    (1 + z), their product and the square root: (3 / 2 + 1) u, times w / pi: 0.8; the products d * (.) and w * c: 1 + 0.32; the
    sum: u (|d| pi + w) / pi <= 1.32; the division by pi and the rounding of pi itself: 1 + 1.  Sum 11.76: c = 12, fit = 0.
    Nothing here was tuned to a measurement; the observed maxima of error / bound are recorded in docs/HISTORY.md."""
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    lo, hi, e64 = np.asarray(y_min, np.float64), np.asarray(y_max, np.float64), float(dtype(e))
    w = np.abs(hi - lo) / 2
    S = np.maximum(np.maximum(np.abs(lo), np.abs(hi)), np.maximum(abs(e64), w))
    return C_BOUND[form] * u * S + FIT.get(form, 0.0) * w


def band_f32_numpy(y_min, y_max, e):
    """The fp32 band expression of csrc/wagg_common.h restated in NumPy float32 with IEEE division and square root and
    separately rounded multiply-adds: a check of :func:`bound` ("ieee" plus the fit), not of the kernel."""
    f = np.float32
    lo, hi, e = np.asarray(y_min, f), np.asarray(y_max, f), f(e)
    M, w = f(0.5) * (hi + lo), f(0.5) * (hi - lo)
    d = M - e
    az = np.minimum(np.abs(-d / w), f(1))
    t = f(1) - az
    p = np.full(lo.shape, f(7.577220821985975e-05))
    for c in (-0.0003951705584768206, 0.0010792884277179837, -0.002406827174127102, 0.005977150052785873,
              -0.022534651681780815, 0.31830987334251404):
        p = (p.astype(np.float64) * az + np.float64(f(c))).astype(f)          # one rounding per step, like an fma
    q = np.sqrt(t) * t
    return (w.astype(np.float64) * (q * p) + np.maximum(d, f(0))).astype(f)


# ---- fields of the GPU module ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(dtype, kelvin, which):
    """The cases of every threshold in one fixed shuffled list: ``which`` = "finite" (no NaN, no inf), "nan" (with the NaN
    classes) or "all" (with the +-inf group too).  ``kelvin``: raw values for ``offset = -273.15`` (the four degree-C
    thresholds); otherwise values for ``offset = 0`` (all five)."""
    cats = [catalogue_kelvin(dtype, e) for e in CELSIUS_THRESHOLDS] if kelvin else [catalogue(dtype, e) for e in THRESHOLDS]
    lo, hi = np.concatenate([c.tasmin for c in cats]), np.concatenate([c.tasmax for c in cats])
    inf = np.concatenate([c.inf for c in cats])
    keep = np.ones(len(lo), bool)
    if which != "all":
        keep &= ~inf
    if which == "finite":
        keep &= np.isfinite(lo) & np.isfinite(hi)
    lo, hi = lo[keep], hi[keep]
    perm = np.random.default_rng(12).permutation(len(lo))
    lo, hi = lo[perm], hi[perm]
    lo.setflags(write=False), hi.setflags(write=False)
    return lo, hi


def field_index(T, G, E):
    """``case[(g + 7 t) mod E]``: every case visits different cells of a chunk, both halves of an image row, the full
    64-timestep item and the tail"""
    return (np.arange(G)[None, :] + 7 * np.arange(T)[:, None]) % E
