"""Layouts for calling the row-list reductions (wagg_*_reduce_f32 / _f64 and wagg_quantile_select_f32 / _f64, include/wagg.h) as
the C-ABI allows them and the binding never does: a pitched result (ldo > n, out_pstride > P * ldo) at an odd base, fields that
are views into poisoned buffers, a field base that is one element off a 16-byte boundary, a workspace smaller than the family's
own *_work_bytes -- or, for the family that has none and promises to ignore the argument, a workspace that must stay untouched.
Nothing here needs a GPU: tests/test_rowlist_layout_host.py checks this module, tests/test_gpu_rowlist_layout.py runs it.

FAMILIES is the case table: one row per family -- nine: eight reductions and the period quantiles -- with its entry symbol, the
middle of its argument list, its planes, its engine twin and its
reference -- the plain restatements the families' own tests use, imported, on the unpoisoned logical field.

The field of a call: GUARD elements, the (T, ldx) body, GUARD elements.  Listed, in-season cells hold the logical values; the
pad columns [n, ldx), the rows no list names, the out-of-season days of listed rows and both guards hold a rotating poison
(NaN, +inf, -inf, 1e30): a kernel that reads one of them adds NaN or inf, counts a day or sets the status word.
The result of a call lies inside a buffer filled with a NaN payload no arithmetic produces, with ldo = n + 5 and
out_pstride = P * ldo + 7; everything outside [k][p][0:n] must keep that payload bit for bit."""
import collections
import ctypes as C

import numpy as np

from tests import exposure_ref as ER
from tests.quantile_ref import quantile_ref
from tests.rolling_ref import rolling_ref
from tests.spell_ref import in_season, spell_ref
from tests.test_gpu_bins import _restate
from tests.test_gpu_hinge import TAIL_KNOTS, _terms, _Worst
from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok
from tests.test_gpu_periods import _ok, _psum
from tests.test_gpu_seasons import _mixed_cells, _pack

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
RTOL = {F32: RTOL32, F64: RTOL64}
KELVIN = -273.15
GUARD = 4096
POISON = (np.nan, np.inf, -np.inf, 1e30)
SENTINEL = {4: 0x7FC5A5A5, 8: 0x7FF8A5A5A5A5A5A5}      # quiet NaNs with a payload: no sum, count or extreme has these bits
NS = (5, 257, 1029)
ROUTES = ("1", "2", "3", "3b")                         # 16-byte pieces | ldx % V == 1 | every base one element off | X2's base only
WORKS = ("full", "three", "one", "none")               # the family's *_work_bytes | 3 parts | one part and 8 bytes | NULL

# the spells' small shape (tests/test_gpu_rolling.py): 9, 8 and 0 entries, a gap at row 4; rows 4 and 18..22 are in no list
SMALL = (23, np.array([0, 9, 17, 17]), np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]))
# ONE period of 70 entries: the split path (8 parts on every route); row 41 is in no list, row 5 is listed twice
SPLIT = (70, np.array([0, 70]), np.concatenate([np.arange(41), np.arange(42, 70), [5]]))
# ONE period of 512 entries over 64 rows, for n = 4097 only: the smallest shape at which the ROUTE decides the parts.  One cell
# per lane makes 17 column blocks, so the rule wants ceil(1024 / 17) = 61 parts; 16-byte pieces make 5 (fp32) or 9 (fp64) and
# hit the cap of 64 -- the family's *_work_bytes holds 64, and a call on the one-cell route must leave the last three alone
LONG = (64, np.array([0, 512]), np.arange(512) % 64)
LISTS = {"small": SMALL, "split": SPLIT, "long": LONG}
SPLIT_PARTS = 8
LONG_N, LONG_PARTS = 4097, {True: 64, False: 61}       # by "16-byte pieces?"
# the shape above on the 16-byte route and with tasmax alone off its boundary -- for the calls that read tasmax
LONG_CASES = (("long", "1", LONG_N, False, 0), ("long", "3b", LONG_N, True, 1))

# (lists, route, n, with a season, out_dev's offset from a 16-byte boundary in elements): paired, not multiplied -- every
# route meets every n, both list shapes, both season forms and both result bases
CASES = (
    ("small", "1", 5, True, 0), ("small", "2", 1029, False, 1), ("small", "3", 257, True, 0), ("small", "1", 257, False, 1),
    ("small", "3b", 1029, True, 0), ("small", "2", 5, True, 1),
    ("split", "1", 1029, True, 1), ("split", "2", 257, False, 0), ("split", "3", 5, True, 1), ("split", "3b", 257, False, 1),
    ("split", "1", 257, False, 0), ("split", "3", 1029, False, 0), ("split", "3b", 5, True, 0),
)
CASE_IDS = ["%s-r%s-n%d-%s-o%d" % (ls, r, n, "season" if s else "plain", o) for ls, r, n, s, o in CASES]


def works_for(lists):
    """the workspaces a case runs with: a small list never splits, so only the full size (0: NULL) and one that must stay
    untouched; the split shape takes all four"""
    return ("full", "three") if lists == "small" else WORKS


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def vec(dtype):
    return 16 // np.dtype(dtype).itemsize


def ldx_for(route, n, dtype):
    """the row pitch of a route: the next multiple of V above n, or the next value above n that is 1 mod V -- at least one pad
    column either way"""
    V = vec(dtype)
    ld = n + 1
    while ld % V != (1 if route == "2" else 0):
        ld += 1
    return ld


def shifts_for(route):
    """(X's, X2's) offset from a 16-byte boundary, in elements"""
    return {"1": (0, 0), "2": (0, 0), "3": (1, 1), "3b": (0, 1)}[route]


def is_wide(route, dtype, n, two_fields):
    """rowlist_geometry's rule restated: 16-byte pieces iff ldx % V == 0 and every field the call reads starts on 16 bytes"""
    sx, s2 = shifts_for(route)
    return ldx_for(route, n, dtype) % vec(dtype) == 0 and sx == 0 and (s2 == 0 or not two_fields)


def poisoned(X, live, ldx, shift):
    """(flat buffer, index of the view's first element): the logical (T, n) field X as a (T, ldx) body at GUARD + shift in a
    buffer of rotating poison; only the cells of `live` hold X"""
    T, n = X.shape
    assert ldx > n and live.shape == X.shape
    total = GUARD + shift + T * ldx + GUARD
    i = np.arange(total)
    with np.errstate(over="ignore"):
        flat = np.asarray(POISON, dtype=X.dtype)[(i + i // ldx) % 4]        # (one step on along a row and from row to row)
    start = GUARD + shift
    body = flat[start:start + T * ldx].reshape(T, ldx)
    body[:, :n][live] = X[live]
    return flat, start


def zero_padded(X, ldx, shift):
    """the twin's buffer: the whole logical field at the same pitch and base offset, pads 0"""
    T, n = X.shape
    flat = np.zeros(shift + T * ldx + 16, dtype=X.dtype)
    flat[shift:shift + T * ldx].reshape(T, ldx)[:, :n] = X
    return flat, shift


OutLayout = collections.namedtuple("OutLayout", "planes P n ldo pstride start total")


def out_layout(planes, P, n, off):
    ldo = n + 5
    pstride = P * ldo + 7
    start = GUARD + off
    return OutLayout(planes, P, n, ldo, pstride, start, start + planes * pstride + GUARD)


def inside_index(lay):
    """(planes, P, n) flat indices of out[k][p][j]"""
    k, p, j = np.ogrid[:lay.planes, :lay.P, :lay.n]
    return lay.start + k * lay.pstride + p * lay.ldo + j


def per_part(planes, P, n):
    return 8 * planes * P * n


def full_work_bytes(L, fam, v, n, P, n_rows):
    """the "full" workspace of a call: the family's own *_work_bytes -- or, for a family without one (fam.work_bytes is None: it
    ignores work / work_bytes), a fixed non-zero size, three parts, every byte of which must keep its sentinel"""
    if fam.work_bytes is None:
        return 3 * per_part(v.planes, P, n)
    return int(getattr(L, fam.work_bytes)(n, P, n_rows, work_count(fam, v)))


def symbol(fam, dtype):
    """the family's entry point for an element type"""
    return "%s_%s" % (fam.entry, "f32" if np.dtype(dtype) == np.dtype(F32) else "f64")


def work_bytes_of(kind, full, planes, P, n):
    return {"full": full, "three": 3 * per_part(planes, P, n), "one": per_part(planes, P, n) + 8, "none": 0}[kind]


def rule_split(n, P, n_rows, v):
    """rowlist_split restated (csrc/wagg_rowlist.h: RL_BLOCK 256, RL_TARGET_BLOCKS 1024, RL_MAX_SPLIT 64, RL_MIN_ROWS_PER_PART
    8): the parts that fill the device, no more than the mean list length / 8 and 64; `v` cells per lane"""
    blocks = -(-n // (256 * v)) * P
    if blocks <= 0 or blocks >= 1024:
        return 1
    want = min(-(-1024 // blocks), n_rows // P // 8, 64)
    return 1 if want < 2 else want


def expected_split(kind, full, planes, P, n, n_rows, v):
    """the parts rowlist_geometry cuts a list into: what the rule wants for `v` cells per lane, cut to what the workspace holds"""
    rule = rule_split(n, P, n_rows, v)
    holds = work_bytes_of(kind, full, planes, P, n) // per_part(planes, P, n)
    return 1 if rule < 2 or holds < 2 else min(rule, holds)


# ---- data ----------------------------------------------------------------------------------------------------------------------
Data = collections.namedtuple("Data", "X H T n rb rows P doy win m01 seasoned live dtype")


def make_data(lists, n, dtype, seasoned, seed=0, inf_at=None):
    """Kelvin tasmin-like X and tasmax-like H with the NaN cases of the families' tests (a NaN in season in an open cell, a cell
    that is NaN on every day, a NaN in either field alone and in both, one inside a run), days without a diurnal range, a cell
    wholly below 0 C and one wholly above 35 C (the exposure bins' exact cases); day-of-year and mixed windows; `live`: the cells
    a call may read.  `inf_at`: a (row, cell) that becomes +inf in X -- the control of the status word."""
    T, rb, rows = LISTS[lists]
    rng = np.random.default_rng(1000 * T + n + seed)
    X = (280 + 15 * rng.standard_normal((T, n))).astype(dtype)
    H = (X + rng.uniform(0, 12, X.shape)).astype(dtype)
    flat = rng.random((T, n)) < 0.03
    H[flat] = X[flat]
    X[:, 2], H[:, 2] = 273.15 + rng.uniform(-9.0, -5.0, T), 273.15 + rng.uniform(-4.0, -1.0, T)
    X[:, 3], H[:, 3] = 273.15 + rng.uniform(36.0, 38.0, T), 273.15 + rng.uniform(39.0, 42.0, T)
    X[0, 0] = np.nan
    X[7, 1] = np.nan
    H[2, n // 2] = np.nan
    X[3, n - 1] = H[3, n - 1] = np.nan
    if n > 6:
        X[:, 6] = np.nan
    if inf_at is not None:
        X[inf_at] = np.inf
    doy = np.arange(100, 100 + T)
    win = _pack(*_mixed_cells(n, doy))
    if lists == "small":
        doy[12] = 2000                                   # a listed row whose day is in no season
    m01 = np.stack([in_season(int(d), win) for d in doy]).astype(np.float64)
    listed = np.zeros(T, dtype=bool)
    listed[rows] = True
    live = listed[:, None] & ((m01 > 0) if seasoned else np.ones((T, n), dtype=bool))
    return Data(X, H, T, n, rb, rows, len(rb) - 1, doy, win, m01 if seasoned else np.ones((T, n)), seasoned, live, dtype)


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def _dbl(v):
    return np.ascontiguousarray(v, dtype=np.float64)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


Variant = collections.namedtuple("Variant", "id two_fields planes p")
# name: the family; entry: its symbol without _f32 / _f64 (wagg_<name>_reduce for all but the quantiles); work_bytes: the export, or
# None for a family that has none and ignores work / work_bytes (it never splits: splits is False); count_extra: what *_work_bytes takes beyond the planes (edges);
# season_args: "none" (no doy / win in the list), "always", "optional"; splits: does a list ever go through the workspace;
# counting: the same bits under every split (integers, or never split); middle(v, p): the arguments between the common head and
# the common tail, p being build_args' dict (the arrays they point into are returned too and must outlive the call); twin(engine, X, X2, d, v): the binding's call;
# check(got, d, v): asserts the (planes, P, n) result against the reference
Family = collections.namedtuple("Family", "name entry work_bytes count_extra four_plane season_args splits counting variants middle twin check")

THR2 = [12.5, 3.0]
THR9 = [float(t) for t in np.linspace(-10.0, 30.0, 9)]
BIN_EDGES = [-np.inf, -12.0, 0.0, 5.5, 11.0, 19.25, 30.0, 35.0, 40.0, np.inf]
EXP_EDGES = [-np.inf, 0.0, 5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0, np.inf]
KNOTS9 = [12.0, -5.0, 28.0, 0.0, 20.0, 4.0, 24.0, 8.0, 16.0]
TAIL_A = [0.5, -1.25, 2.0, -0.75, 1.5, -2.5, 0.25, 3.0, -1.0]
TAIL_B = [-1.5, 0.75, -2.0, 1.25, -0.5, 2.5, -0.25, -3.0, 1.0]
SPELL_THR = [7.0, -5.0, 20.0]


def _season_kw(d):
    return {"doy": d.doy, "windows": d.win} if d.seasoned else {}


def _mid_four(v, p=None):
    import climate_toolbox_amd._lib as _lib
    if v.id == "poly":
        return [_lib.XF_POLY, KELVIN, 1, v.planes, None, 0], ()
    thr = _dbl(v.p)
    return [_lib.XF_EDD, KELVIN, 1, 1, _dp(thr), len(thr)], (thr,)


def _four_kw(X2, v):
    return {"poly": (KELVIN, 1, v.planes)} if v.id == "poly" else {"X2": X2, "edd": (KELVIN, v.p)}


def _check_edd(got, d, thresholds):
    from oracle import ref_numpy as O
    cmin, cmax = d.X + d.dtype(KELVIN), d.H + d.dtype(KELVIN)
    for k, e in enumerate(thresholds):
        o = np.nan_to_num(O.snyder_edd_values(cmin, cmax, e), nan=0.0)
        _rel_ok(got[k], _psum(d.m01 * o, d.rb, d.rows), RTOL[d.dtype], scale=0.05 * d.T)


def _check_four(got, d, v):
    from oracle import ref_numpy as O
    if v.id == "edd":
        return _check_edd(got, d, v.p)
    for k in range(v.planes):
        f = np.nan_to_num(O.tas_poly_values(d.X, k + 1), nan=0.0)
        _ok(got[k], _psum(d.m01 * f, d.rb, d.rows), RTOL[d.dtype], _psum(d.m01 * np.abs(f), d.rb, d.rows))


def exact(got, want, what):
    """equal as numbers, NaN exactly where the restatement has NaN"""
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, "%r: %d values differ, first at (plane, period, cell) %r: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _mid_list(v, p=None):
    a = _dbl(v.p)
    return [_dp(a), len(a)], (a,)


def _check_bins(got, d, v):
    exact(got.astype(np.float64), _restate(d.X, d.m01, d.rb, d.rows, v.p, KELVIN), ("bins", d.n))


def _hinge_p(v):
    power, side, tail = v.p
    return power, side, ((TAIL_KNOTS, TAIL_A, TAIL_B) if tail else None)


def _mid_hinge(v, p=None):
    import climate_toolbox_amd._lib as _lib
    power, side, tail = _hinge_p(v)
    k = _dbl(KNOTS9)
    keep = [k] + ([_dbl(t) for t in tail] if tail else [])
    t = keep[1:] if tail else [None, None, None]
    return [_dp(k), len(k), power, _lib.HINGE_BELOW if side == "below" else _lib.HINGE_ABOVE] + [_dp(a) for a in t], tuple(keep)


def _check_hinge(got, d, v):
    power, side, tail = _hinge_p(v)
    daily = _terms(d.X, KELVIN, np.concatenate([KNOTS9, TAIL_KNOTS]), power, side)
    sums = np.stack([_psum(p * d.m01, d.rb, d.rows) for p in daily])
    ref, hA, hB = sums[:9], sums[9], sums[10]
    A = ref
    if tail:
        a, b = np.asarray(TAIL_A)[:, None, None], np.asarray(TAIL_B)[:, None, None]
        ref, A = (ref + a * hA) + b * hB, ref + np.abs(a) * hA + np.abs(b) * hB
    _Worst().close(got, ref, A, RTOL[d.dtype], ("hinge", d.n, v.id))


def _check_exposure(got, d, v):
    want = ER.exposure_bins(d.X, d.H, KELVIN, v.p, d.rb, d.rows, d.m01)
    D = ER.counted_days(d.X, d.H, d.rb, d.rows, d.m01)
    g = got.astype(np.float64)
    assert np.isfinite(g).all()
    bad = np.argwhere(np.abs(g - want) > RTOL[d.dtype] * D[None])
    assert len(bad) == 0, "exposure: %d values beyond tol * D, first at (bin, period, cell) %r: got %r, want %r" % (
        len(bad), tuple(bad[0]), g[tuple(bad[0])], want[tuple(bad[0])])
    exact(g[:, :, 2:4], want[:, :, 2:4], ("exposure: the cells wholly below 0 C and wholly above 35 C", d.n))
    assert (want[1:, :, 2] == 0).all() and (want[:-1, :, 3] == 0).all() and (want[0, :, 2] == D[:, 2]).all() and (want[-1, :, 3] == D[:, 3]).all()


def _mid_spell(v, p=None):
    import climate_toolbox_amd._lib as _lib
    L, stat, side = v.p
    a = _dbl(SPELL_THR)
    return [_dp(a), len(a), L, {"days": _lib.SPELL_DAYS, "events": _lib.SPELL_EVENTS, "longest": _lib.SPELL_LONGEST}[stat],
            1 if side == "below" else 0], (a,)


def _check_spell(got, d, v):
    L, stat, side = v.p
    sk = (d.doy, d.win) if d.seasoned else (None, None)
    exact(got.astype(np.float64), spell_ref(d.X, d.rb, d.rows, KELVIN, SPELL_THR, L, stat, side, *sk), ("spell", d.n, v.id))


def _mid_roll(v, p=None):
    import climate_toolbox_amd._lib as _lib
    lengths, stat, of = v.p
    w = np.ascontiguousarray(lengths, dtype=np.int32)
    return [w.ctypes.data_as(C.POINTER(C.c_int32)), len(w), _lib.ROLL_MAX if stat == "max" else _lib.ROLL_MIN,
            _lib.ROLL_MEAN if of == "mean" else _lib.ROLL_SUM], (w,)


def _check_roll(got, d, v):
    lengths, stat, of = v.p
    sk = (d.doy, d.win) if d.seasoned else (None, None)
    exact(got, rolling_ref(d.X, d.rb, d.rows, KELVIN, lengths, stat, of, *sk), ("rolling", d.n, v.id))


Q8 = [0.0, 0.05, 1.0 / 3.0, 0.5, 0.9, 0.95, 1.0, 0.5]
Q16 = [0.5, 0.0, 1.0, 0.05, 0.95, 0.99, 0.01, 1.0 / 3.0, 2.0 / 3.0, 0.25, 0.75, 0.5, 0.1, 0.9, 0.125, 0.999]
QUANT_ROWS_MAX = 1024


def longest_list(rb):
    return int(np.diff(np.asarray(rb)).max())


def _quant_max_rows(v, longest):
    """a variant's max_rows: its own, or (None) the longest list of the call"""
    return longest if v.p[2] is None else v.p[2]


def _mid_quantile(v, p):
    import climate_toolbox_amd._lib as _lib
    method, q, _ = v.p
    a = _dbl(q)
    return [_dp(a), len(a), {"linear": _lib.QUANT_LINEAR, "lower": _lib.QUANT_LOWER, "higher": _lib.QUANT_HIGHER}[method],
            _quant_max_rows(v, p["longest"])], (a,)


def _check_quantile(got, d, v):
    method, q, _ = v.p
    sk = (d.doy, d.win) if d.seasoned else (None, None)
    exact(got, quantile_ref(d.X, d.rb, d.rows, KELVIN, q, method, *sk), ("quantile", d.n, v.id))


_FOUR = (Variant("poly", False, 3, None), Variant("edd", True, 2, THR2))
FAMILIES = {f.name: f for f in (
    Family("period", "wagg_period_reduce", "wagg_period_reduce_work_bytes", 0, True, "none", True, False, _FOUR, _mid_four,
           lambda e, X, X2, d, v: e.period_reduce(X, d.rb, d.rows, **_four_kw(X2, v)), _check_four),
    Family("season", "wagg_season_reduce", "wagg_season_reduce_work_bytes", 0, True, "always", True, False, _FOUR, _mid_four,
           lambda e, X, X2, d, v: e.season_reduce(X, d.rb, d.rows, d.doy, d.win, **_four_kw(X2, v)), _check_four),
    Family("edd_ladder", "wagg_edd_ladder_reduce", "wagg_edd_ladder_work_bytes", 0, False, "optional", True, False, (Variant("thr9", True, 9, THR9),), _mid_list,
           lambda e, X, X2, d, v: e.edd_ladder_reduce(X, X2, d.rb, d.rows, KELVIN, v.p, **_season_kw(d)),
           lambda got, d, v: _check_edd(got, d, v.p)),
    Family("bin_days", "wagg_bin_days_reduce", "wagg_bin_days_work_bytes", 1, False, "optional", True, True, (Variant("bins9", False, 9, BIN_EDGES),), _mid_list,
           lambda e, X, X2, d, v: e.bin_days_reduce(X, d.rb, d.rows, KELVIN, v.p, **_season_kw(d)), _check_bins),
    Family("hinge", "wagg_hinge_reduce", "wagg_hinge_work_bytes", 0, False, "optional", True, False,
           (Variant("p1-above", False, 9, (1, "above", False)), Variant("p2-below-tail", False, 9, (2, "below", True))), _mid_hinge,
           lambda e, X, X2, d, v: e.hinge_reduce(X, d.rb, d.rows, KELVIN, KNOTS9, power=_hinge_p(v)[0], side=_hinge_p(v)[1],
                                                 tail=_hinge_p(v)[2], **_season_kw(d)), _check_hinge),
    Family("exposure", "wagg_exposure_reduce", "wagg_exposure_work_bytes", 1, False, "optional", True, False, (Variant("bins9", True, 9, EXP_EDGES),), _mid_list,
           lambda e, X, X2, d, v: e.exposure_reduce(X, X2, d.rb, d.rows, KELVIN, v.p, **_season_kw(d)), _check_exposure),
    Family("spell", "wagg_spell_reduce", "wagg_spell_work_bytes", 0, False, "optional", False, True,
           (Variant("days-above", False, 3, (2, "days", "above")), Variant("events-below", False, 3, (2, "events", "below"))), _mid_spell,
           lambda e, X, X2, d, v: e.spell_reduce(X, d.rb, d.rows, KELVIN, SPELL_THR, min_length=v.p[0], stat=v.p[1], side=v.p[2],
                                                 **_season_kw(d)), _check_spell),
    # a window above 8 days runs one cell per lane whatever the alignment: [3, 16] meets route 1 like every other
    Family("rolling", "wagg_rolling_reduce", "wagg_rolling_work_bytes", 0, False, "optional", False, True,
           (Variant("ring8", False, 5, ([1, 2, 3, 5, 8], "max", "mean")), Variant("ring16", False, 2, ([3, 16], "min", "sum"))), _mid_roll,
           lambda e, X, X2, d, v: e.rolling_reduce(X, d.rb, d.rows, KELVIN, v.p[0], stat=v.p[1], of=v.p[2], **_season_kw(d)), _check_roll),
    # no *_work_bytes: work / work_bytes are ignored.  8 planes with max_rows = the longest list; 16 planes (two quantiles a lane in
    # fp32) with max_rows at the limit, 128 KiB of LDS for a list of 9 or 70 entries
    Family("quantile", "wagg_quantile_select", None, 0, False, "optional", False, True,
           (Variant("linear-q8", False, 8, ("linear", Q8, None)), Variant("higher-q16", False, 16, ("higher", Q16, QUANT_ROWS_MAX))),
           _mid_quantile,
           lambda e, X, X2, d, v: e.quantile_select(X, d.rb, d.rows, KELVIN, v.p[1], method=v.p[0],
                                                    max_rows=_quant_max_rows(v, longest_list(d.rb)), **_season_kw(d)), _check_quantile),
)}


def seasoned_for(fam, seasoned):
    """does this family's call of a case carry a season?"""
    return {"none": False, "always": True, "optional": seasoned}[fam.season_args]


def variants_for(fam, route):
    """the variants a route runs: "3b" moves X2's base alone, which only a call that reads X2 can tell from route 1"""
    return [v for v in fam.variants if route != "3b" or v.two_fields]


def build_args(fam, v, p):
    """(the entry point's argument list, what must outlive the call) from the pointers and sizes `p`: a dict with X, X2, T, n,
    ldx, rb, rows, P, n_rows, doy, win (None without a season), flags, out, ldo, pstride, status, work, work_bytes, stream, and
    longest: the entries of the longest list (a host integer, for a middle that bounds it)"""
    vp = lambda a: None if a is None else C.c_void_p(a)
    mid, keep = fam.middle(v, p)
    if fam.four_plane:
        fields = [vp(p["X"]), vp(p["X2"]) if v.two_fields else None]
    else:
        fields = [vp(p["X"])] + ([vp(p["X2"])] if v.two_fields else [])
    head = fields + [p["T"], p["n"], p["ldx"], vp(p["rb"]), vp(p["rows"]), p["P"], p["n_rows"]]
    if fam.season_args != "none":
        head += [vp(p["doy"]), vp(p["win"])]
    if not fam.four_plane:
        head.append(KELVIN)
    tail = [p["flags"], vp(p["out"]), p["ldo"], p["pstride"], vp(p["status"]), vp(p["work"]), p["work_bytes"], p["stream"]]
    return head + mid + tail, keep


def work_count(fam, v):
    """what the family's *_work_bytes takes as its last argument"""
    return v.planes + fam.count_extra
