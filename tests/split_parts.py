"""The split form of the fp32 full-form contraction, restated in NumPy from the comments at the head of
csrc/wagg_dense_split.inc, and the builders of the cases tests/test_gpu_split_parts.py runs (no GPU here; checked by
tests/test_split_parts_host.py).

The form: row t of X is scaled by 2^ex[t] so that its largest finite |x| lies in [2^14, 2^15), column r of W by 2^ew[r]
likewise; each scaled value y becomes an f16 high part hi = f16(y) and an f16 low part lo = f16(y - hi) (round to nearest
even; NaN counts 0, +-inf keeps hi = +-inf and lo = 0), and

    out[t, r] = 2^-(ex[t] + ew[r]) sum_k (xh wl + xl wh + xh wh) / den[r]            (`expected`)

with the sum in fp32 on the device and in fp64 here.  `true_quotient` is sum_k x w / den in fp64.

ONE_TERM, the bound of the two-part impulse probe, derived operation by operation
-----------------------------------------------------------------------------------
Row g of the probe holds one amplitude a in cell g, so out[g, r] has ONE term: a W[g, r] / den[r].  Write X = a 2^ex,
V = w 2^ew with w = fl32(W[g, r]), u = 2^-24 (half an fp32 ulp, relative), h = 2^-11 (half an f16 ulp, relative).

  1  W[g, r] -> w, the fp32 weight the plan stores:                                  u |a W / den|
  2  X = xh + xl exactly: a two-part amplitude has a 22-bit significand (`two_part`)   0
  3  V = wh + wl + rho: |V - wh| <= h |V|, wl = f16(V - wh) and V - wh is a normal f16
     (or 0), so |rho| <= h |V - wh| <= 2^-22 |V|; the term X rho is lost:            2^-22 |X V|
  4  the products xh wl, xl wh, xh wh of 11-bit parts have 22 bits: exact in fp32      0
  5  xl wl is dropped: |xl| <= h |X|, |wl| <= h (1 + h) |V|:                          2^-22 (1 + 2^-11) |X V|
  6  two fp32 additions (every other k adds an exact 0): s1 = xh wl + xl wh with
     |s1| <= 2 h (1 + h) |X V|, then s2 = s1 + xh wh with |s2| <= (1 + 2^-20) |X V|:  u (2^-10 + 1 + 2^-19) |X V|
  7  the k slices of the reduce add exact zeros; ldexp by -(ex + ew) is exact while
     the result is normal                                                            0
  8  den -> fp32 and one division:                                                   2 u (1 + 2 u) of the quotient

  sum = 2^-22 + 2^-22 (1 + 2^-11) + 4 u + u 2^-10 + O(u^2) < 2^-21 + 2^-22 + 2^-32 = ONE_TERM = 7.16e-7 <= 2^-20,

relative to |a| |W[g, r]| / |den[r]| -- the weight under test, not the column's largest.  Nothing in it was measured.

Step 3 needs V - wh to be 0 or a NORMAL f16.  V - wh is a multiple of the fp32 ulp of V, 2^(E - 23) for |V| in
[2^E, 2^(E + 1)), so it is subnormal in f16 (below 2^-14) only when E < 9: weights below 2^-5 of their column's scaled
range, |w| < 2^(-5 - ew).  For those the documented absolute term is added: 2^-36 of the column's largest |w|, times
|a| / |den| (`one_term_tol`).  In the tables used here that is: no weight of the segment tables of
tests/test_gpu_dense_forms_small.py (uniform(0.1, 1), pair sums below 3: every w is above 2^-5 of its column's range), and
in `host_matrix` only weights of the SMALL_COLS columns, those made 2^-13 or less of the column's largest (E < 9 is
necessary, not sufficient: `floor_mask` marks the weights whose V - wh really is subnormal; the host test prints how many).

The two-cell rows compare with `expected` itself, which already leaves out rho and xl wl: what is left is the fp32
additions, den and the division, below 12 u of |t1| + |t2| -- inside the sum of the two one-term bounds that the issue
asks for."""
import math

import numpy as np

F32 = np.float32
ONE_TERM = 2.0 ** -21 + 2.0 ** -22 + 2.0 ** -32
assert ONE_TERM <= 2.0 ** -20
FLOOR = 2.0 ** -36                                               # the floor of subnormal low parts
FLT_MAX = float(np.finfo(np.float32).max)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def split_exp(m):
    """the exponent that brings a maximum m > 0 into [2^14, 2^15); 0 for m = 0 (elementwise)"""
    m = np.asarray(m, dtype=np.float64)
    _, e = np.frexp(m)
    return np.where(m > 0, 15 - e, 0).astype(np.int64)


def finite_max(A, axis):
    """max |a| along `axis`, NaN counting 0 and +-inf left out"""
    a = np.abs(np.asarray(A, dtype=np.float64))
    return np.where(np.isfinite(a), a, 0.0).max(axis)


def parts(v, e):
    """(hi, lo) in fp64 of y = v 2^e: hi = f16(y), lo = f16(y - hi); NaN -> (0, 0), +-inf -> (+-inf, 0)"""
    v = np.asarray(v, dtype=np.float64)
    y = np.ldexp(np.where(np.isnan(v), 0.0, v), np.broadcast_to(np.asarray(e, dtype=np.int64), v.shape).astype(np.int32))
    with np.errstate(over="ignore", invalid="ignore"):
        hi = y.astype(np.float16).astype(np.float64)
        lo = np.where(np.isinf(hi), 0.0, (y - hi).astype(np.float16).astype(np.float64))
    return hi, lo


def scales(X, W):
    return split_exp(finite_max(X, 1)), split_exp(finite_max(W, 0))


def expected(X, W, den, mutate=None):
    """The split form's value per (t, r) in fp64.  X (T, G) and W (G, R) hold fp32 values.  `mutate` (the host module's
    sensitivity checks): "xl0" zeroes xl, "pair" pairs xl of cell k with wh of cell k ^ 1, "half" swaps the low parts of the
    two halves of a piece (k and k + 16 of a k tile), "ex1" is off by one in the final ldexp."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    ex, ew = scales(X, W)
    xh, xl = parts(X, ex[:, None])
    wh, wl = parts(W, ew[None, :])
    xl_for_wh = xl
    if mutate == "xl0":
        xl_for_wh = np.zeros_like(xl)
    elif mutate in ("pair", "half"):
        G = X.shape[1]
        Gp = -(-G // 32) * 32
        pad = np.zeros((X.shape[0], Gp))
        pad[:, :G] = xl
        k = np.arange(Gp)
        xl_for_wh = pad[:, k ^ 1 if mutate == "pair" else k ^ 16][:, :G]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = xh @ wl + xl_for_wh @ wh + xh @ wh
        e = ex[:, None] + ew[None, :] + (1 if mutate == "ex1" else 0)
        return np.ldexp(s, (-e).astype(np.int32)) / np.asarray(den, dtype=np.float64)[None, :]


def true_quotient(X, W, den):
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (np.where(np.isnan(X), 0.0, X) @ W) / np.asarray(den, dtype=np.float64)[None, :]


def floor_mask(W):
    """the weights whose scaled low part is subnormal in f16 (see the module's docstring)"""
    W = np.asarray(W, dtype=np.float64)
    _, ew = scales(np.zeros((1, W.shape[0])), W)
    V = np.ldexp(W, np.broadcast_to(ew[None, :], W.shape).astype(np.int32))
    r = V - V.astype(np.float16).astype(np.float64)
    return (r != 0) & (np.abs(r) < 2.0 ** -14)


def one_term_tol(a, W, den):
    """the probe's tolerance per (g, r): ONE_TERM |a_g| |W[g, r]| / |den[r]|, plus FLOOR max|W[:, r]| |a_g| / |den[r]| for
    the weights of `floor_mask`"""
    W = np.asarray(W, dtype=np.float64)
    a = np.abs(np.asarray(a, dtype=np.float64))[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        tol = ONE_TERM * a * np.abs(W) / np.abs(den)[None, :]
        return tol + np.where(floor_mask(W.astype(F32)), FLOOR * finite_max(W, 0)[None, :] * a / np.abs(den)[None, :], 0.0)


# ---- two-part amplitudes -------------------------------------------------------------------------------------------------------
def two_part(G, shift=0, salt=0):
    """a_g, g < G: fp32 values +-2^k (1 + H 2^-10 + L 2^-21) 2^-shift, k cycling through -3 .. 3 and the sign alternating
    as in the power-of-two probe.  H (ten bits) takes every residue and is 1023 -- the high part rounds up to the next
    binade, 2^15 after scaling -- every 64th g; L (eleven bits, odd: the 22-bit significand is used in full) lies in
    [513, 1535]: the scaled value y = 2^14 + 16 H + L / 128 has hi = the nearest multiple of 16 and
    lo = L / 128 (L < 1024) or (L - 2048) / 128, so 4 < |lo| < 12 -- an exact f16 of both signs -- and
    |lo| >= 4 = 2^-13 2^15 > 2^-13 |y| for EVERY g.  Both conditions are asserted."""
    g = np.arange(G) + 1000 * salt
    H = np.where(g % 64 == 63, 1023, (g * 97 + 13) % 1024)
    L = 513 + 2 * ((g * 37 + 5) % 512)
    assert ((L >= 513) & (L <= 1535) & (L % 2 == 1)).all()
    m = 1.0 + H * 2.0 ** -10 + L * 2.0 ** -21
    a = np.where(np.arange(G) % 2 == 0, 1.0, -1.0) * m * 2.0 ** (np.arange(G) % 7 - 3 - shift)
    assert (a.astype(F32).astype(np.float64) == a).all()
    y = np.abs(a) * 2.0 ** split_exp(np.abs(a) * 2.0 ** shift)   # (scaled by the maximum of a row that holds a 2^shift alone)
    hi, lo = parts(y, 0)
    assert (hi + lo == y).all() and (np.abs(lo) >= 2.0 ** -13 * y).all() and (np.abs(lo) >= 2.0 ** -14).all()
    return a


def impulse_field(G):
    """(X, a): T = G rows, row g holds a_g in cell g"""
    a = two_part(G)
    X = np.zeros((G, G), dtype=F32)
    X[np.arange(G), np.arange(G)] = a
    return X, a


def two_cell_field(G):
    """(X, a, a2, g2): row g holds a_g in cell g and a2_g = a two-part amplitude 2^-9 times smaller in cell (g + 17) % G"""
    X, a = impulse_field(G)
    a2 = two_part(G, shift=9, salt=1)
    g2 = (np.arange(G) + 17) % G
    X[np.arange(G), g2] = a2
    assert (np.abs(a2) < np.abs(a) * 2.0 ** -7).all()
    return X, a, a2, g2


# ---- host matrices whose own low parts are large ---------------------------------------------------------------------------------
SMALL_COLS = (1, 4)


def host_matrix(G, R):
    """A (G, R) fp32 matrix for DensePlan.from_host: 30 % zeros, weights uniform(0.1, 1) with all 24 bits of the significand
    in use and the low part of the split at least a quarter of its largest (|V - wh| >= 2^-13 |V|); a few negative; in the
    columns SMALL_COLS every fifth weight is 2^-7 .. 2^-20 of the column's largest (a small weight beside a large one; the
    smallest of them have subnormal low parts: the floor of `one_term_tol`); column R // 2 sums to 0 (+1.5 and -1.5)."""
    rng = np.random.default_rng(77 * G + R)
    top = rng.integers(2 ** 10, 2 ** 11, (G, R))                 # the eleven bits of the high part
    mid = rng.integers(256, 768, (G, R)) * 2 + 1                 # the next eleven: far from 0 and from the rounding point
    low = rng.integers(0, 4, (G, R))
    m = (top * 2.0 ** 13 + mid * 2.0 ** 2 + low) * 2.0 ** -24     # in [0.5, 1), 24 bits
    W = m * 2.0 ** rng.integers(-3, 1, (G, R))                   # [2^-4, 1)
    W[rng.random((G, R)) < 0.3] = 0.0
    W[rng.random((G, R)) < 0.01] *= -1.0
    for c in SMALL_COLS:
        if c < R:
            W[::5, c] *= 2.0 ** -rng.integers(7, 21, len(W[::5, c]))
            W[1, c] = 0.984375                                   # the column's largest
    W[:, R // 2] = 0.0
    W[5, R // 2], W[G - 2, R // 2] = 1.5, -1.5
    W[0, 0] = abs(W[0, 0]) or 0.75
    W32 = W.astype(F32)
    assert (W32 == W).all()
    W32.setflags(write=False)
    return W32


# ---- exponent edges --------------------------------------------------------------------------------------------------------------
EDGE_ROW_NAMES = ("2^-149", "2^-127", "2^-126", "2^-126 (2 - 2^-22)", "1", "2^127", "FLT_MAX", "-FLT_MAX alone", "zeros", "NaN",
                  "-0.0", "FLT_MAX beside 2^-100")


def edge_matrix(G, R):
    """weights uniform[0.25, 0.9375) (24 bits), 30 % zeros, every column sum above 1: sum x w stays below FLT_MAX beside one cell
    of FLT_MAX, and a subnormal numerator's rounding (2^-150 at most) stays 2^-150 after the division"""
    rng = np.random.default_rng(91 * G + R)
    W = rng.uniform(0.25, 0.9375, (G, R)).astype(F32)
    W[rng.random((G, R)) < 0.3] = 0.0
    W[:4] = np.maximum(W[:4], F32(0.25))
    assert (W.astype(np.float64).sum(0) > 1).all() and (W < 0.9375).all()
    W.setflags(write=False)
    return W


def edge_rows(G):
    """The rows of EDGE_ROW_NAMES for G cells: the named value as the row's largest |x| (in cell 7 or G - 3), the other cells
    below it (or as named).  The rows up to 2^127 have cells of both signs, of the row's own magnitude where the format has
    room below it; the rows with FLT_MAX keep sum x w in range (one such cell, weights below 1)."""
    rng = np.random.default_rng(5 * G + 3)
    X = np.zeros((len(EDGE_ROW_NAMES), G), dtype=np.float64)
    sign = rng.choice([-1.0, 1.0], G)
    X[0] = np.where(rng.random(G) < 0.4, sign * 2.0 ** -149, 0.0)
    X[0, 7] = 2.0 ** -149
    X[1] = sign * rng.integers(0, 2 ** 22, G) * 2.0 ** -149
    X[1, G - 3] = -2.0 ** -127
    X[2] = sign * rng.integers(0, 2 ** 23, G) * 2.0 ** -149
    X[2, 7] = 2.0 ** -126
    X[3] = sign * rng.integers(0, 2 ** 24 - 4, G) * 2.0 ** -149
    X[3, G - 3] = 2.0 ** -126 * (2 - 2.0 ** -22)
    X[4] = rng.uniform(-1, 1, G)
    X[4, 7] = -1.0
    X[5] = rng.uniform(-1, 1, G) * 2.0 ** 110
    X[5, G - 3] = 2.0 ** 127
    X[6] = rng.uniform(-1, 1, G) * 2.0 ** 100
    X[6, 7] = FLT_MAX
    X[7, G - 3] = -FLT_MAX
    X[9] = np.nan
    X[10] = -0.0
    X[11] = sign * 2.0 ** -100
    X[11, 7] = FLT_MAX
    X32 = X.astype(F32)
    m = finite_max(X32, 1)
    assert list(m[:8]) == [2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -126 * (2 - 2.0 ** -22), 1.0, 2.0 ** 127, FLT_MAX, FLT_MAX]
    assert list(split_exp(m)[:7]) == [163, 141, 140, 140, 14, -113, -113] and np.signbit(X32[10]).all()
    X32.setflags(write=False)
    return X32


EDGE_COLS = {0: 2.0 ** -140, 1: 2.0 ** -126, 2: 2.0 ** 100}     # column -> its largest weight; column 3 is all zero
EDGE_COL_ZERO = 3
EDGE_ROW_SCALES = (120, 96, 20, 8, 0, -20, -60, -100, -118)


def edge_columns(G, R):
    """(W, X) for the column edges, all values >= 0 (no cancellation: sum x w is as large as sum |x| |w|).  Columns 0, 1, 2
    hold weights up to 2^-140 (subnormal: multiples of 2^-149), 2^-126 and 2^100, column 3 zeros, the others uniform[0.25, 1).
    Row i of X is 2^EDGE_ROW_SCALES[i] times uniform[0.5, 1).  `edge_valid` says which (row, column)
    results count: those whose products, numerator and result are all normal fp32 numbers.  That leaves ex + ew from 48 to 148
    in column 0, 34 .. 146 in column 1, -80 (or below) .. 46 in column 2 and -67 (or below) .. 147 in the ordinary columns: a
    result that is a normal number keeps ex <= 141 and sum x w <= 2^127 keeps ex + ew >= -100, so +-300 cannot be reached
    (the host test asserts these extremes)."""
    assert R > 4
    rng = np.random.default_rng(17 * G + R)
    W = rng.uniform(0.25, 1.0, (G, R))
    W[rng.random((G, R)) < 0.3] = 0.0
    for c, top in EDGE_COLS.items():
        W[:, c] = np.where(W[:, c] > 0, W[:, c] * top, 0.0)
        W[3, c] = top
    W[:, EDGE_COL_ZERO] = 0.0
    W32 = W.astype(F32)
    assert [float(finite_max(W32, 0)[c]) for c in EDGE_COLS] == list(EDGE_COLS.values())
    X = np.stack([rng.uniform(0.5, 1.0, G) * 2.0 ** s for s in EDGE_ROW_SCALES]).astype(F32)
    X[:, 3] = [F32(2.0 ** s) for s in EDGE_ROW_SCALES]           # (a power of two: the row's largest)
    W32.setflags(write=False), X.setflags(write=False)
    return W32, X


def edge_valid(X, W):
    """(t, r) whose every non-zero product |x| |w| is at least 2^-126 (smallest |x| of the row times smallest |w| of the
    column), whose numerator sum |x| |w| is at most 2^126 and whose quotient lies in [2^-120, 2^126]"""
    ax, aw = np.abs(np.asarray(X, dtype=np.float64)), np.abs(np.asarray(W, dtype=np.float64))
    num = ax @ aw
    xmin = np.where(ax > 0, ax, np.inf).min(1)
    wmin = np.where(aw > 0, aw, np.inf).min(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = num / aw.sum(0)[None, :]
        return (xmin[:, None] * wmin[None, :] >= 2.0 ** -126) & (num <= 2.0 ** 126) & (q >= 2.0 ** -120) & (q <= 2.0 ** 126)


def den_format_term(q, den):
    """what rounding den to fp32 can move the quotient q by: |q| |fl32(den) - den| / |fl32(den)| -- 2^-24 |q| for a normal
    den, more for a subnormal one (column 0 of `edge_columns`: den is a multiple of 2^-149 near 2^-133)"""
    den = np.asarray(den, dtype=np.float64)
    d32 = den.astype(F32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(d32 != 0, np.abs(d32 - den) / np.abs(d32), 0.0)
    return np.abs(q) * rel[None, :]


def fsum_check(X, W, den, t, r):
    """`expected` at one (t, r) with math.fsum (an independent order of the sum)"""
    ex, ew = scales(X, W)
    xh, xl = parts(np.asarray(X, dtype=np.float64)[t], ex[t])
    wh, wl = parts(np.asarray(W, dtype=np.float64)[:, r], ew[r])
    s = math.fsum(np.concatenate([xh * wl, xl * wh, xh * wh]).tolist())
    return math.ldexp(s, -int(ex[t] + ew[r])) / float(den[r])
