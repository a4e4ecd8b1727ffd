"""The period quantiles of wagg_quantile_select_* (include/wagg.h), restated in plain NumPy: a Python loop per period and cell,
``np.sort`` of the cell's valid raw elements and the arithmetic of the definition in ``np.float64``, one operation a line so that
nothing can be fused.  Used by tests/test_quantile_host.py and tests/test_gpu_quantile.py.

Below it, the LONG SHAPE those two share (no GPU needed to build it): T = 1040 rows and ONE call with periods of 255, 256, 257,
365, 366, 512, 513, 1023, 1024 and 0 entries -- a year, a leap year, the kernel's limit of 1024 and one short of it, both sides
of the 64 KiB half of its LDS (entry 512) -- every list a seeded permutation of distinct rows of 0..1029 (so the LDS entry index
is not the row index), the 257-entry list naming one row twice, rows 1030..1039 in no list (they hold +inf: a kernel that reads
them raises the status word)."""
import numpy as np

from tests.rolling_ref import WIN_INVERT, WIN_NULL, in_season  # noqa: F401

QUANT_MAX, QUANT_ROWS_MAX = 16, 1024
METHODS = ("linear", "lower", "higher")


def quantile_ref(X, row_begin, rows, offset, q, method="linear", doy=None, windows=None, max_rows=None):
    """``out[k, p, j]`` in ``X``'s dtype.  Entry ``i`` of period ``p``'s list is valid for cell ``j`` when ``t = rows[i]`` lies in
    ``[0, T)``, the cell is in season on ``doy[t]`` (when a season is given) and ``X[t, j]`` is not NaN; a row listed twice counts
    twice.  ``v`` = the valid raw elements sorted, ``m = len(v)``; ``h = float64(m - 1) * q[k]``, ``lo = floor(h)``, ``g = h - lo``;
    linear: ``v[lo]`` where ``g == 0``, else ``v[lo] + (v[lo + 1] - v[lo]) * g`` in float64; lower: ``v[lo]``; higher: ``v[lo]``
    where ``g == 0``, else ``v[lo + 1]``.  The result is that plus ``offset``, rounded once to the dtype; ``m == 0`` gives NaN.
    ``max_rows``: a period whose list holds more entries is NaN throughout (the kernel's confinement under ``checked=True``)."""
    X = np.asarray(X)
    T, n = X.shape
    row_begin, rows = np.asarray(row_begin, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    assert method in METHODS and (doy is None) == (windows is None) and 1 <= len(q) <= QUANT_MAX and ((q >= 0) & (q <= 1)).all()
    P = len(row_begin) - 1
    out = np.full((len(q), P, n), np.nan, dtype=X.dtype)
    off = np.float64(offset)
    for p in range(P):
        lst = rows[row_begin[p]:row_begin[p + 1]]
        if max_rows is not None and len(lst) > max_rows:
            continue
        ts = [int(t) for t in lst if 0 <= t < T]
        if not ts:
            continue
        block = X[ts]                                                            # (entries, n), a row listed twice is there twice
        ok = ~np.isnan(block)
        if doy is not None:
            ok &= np.stack([in_season(int(doy[t]), windows) for t in ts])
        for j in range(n):
            v = np.sort(block[ok[:, j], j]).astype(np.float64)
            m = len(v)
            if m == 0:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                for k in range(len(q)):
                    h = np.float64(m - 1) * q[k]
                    lo = int(np.floor(h))
                    g = h - np.float64(lo)
                    if g == 0.0 or method == "lower":
                        r = v[lo]
                    elif method == "higher":
                        r = v[lo + 1]
                    else:
                        d = v[lo + 1] - v[lo]
                        step = d * g
                        r = v[lo] + step
                    out[k, p, j] = X.dtype.type(r + off)
    return out


LONG_T, LONG_LISTED = 1040, 1030
LONG_LENGTHS = (255, 256, 257, 365, 366, 512, 513, 1023, 1024, 0)
LONG_TWICE = 2                                                                  # the period whose list names one row twice
LONG_KINDS = "abcdef"


def long_lists(seed=5):
    """``(row_begin, rows)`` of the long shape"""
    rng = np.random.default_rng(seed)
    lists = []
    for p, L in enumerate(LONG_LENGTHS):
        if p == LONG_TWICE:
            rows = rng.permutation(LONG_LISTED)[:L - 1]
            rows = np.insert(rows, 100, rows[7])
        else:
            rows = rng.permutation(LONG_LISTED)[:L]
        lists.append(rows)
    return np.concatenate([[0], np.cumsum(LONG_LENGTHS)]), np.concatenate(lists)


def long_field(n, dtype, seed=0):
    """The (1040, n) field of the long shape; column ``j`` is of kind ``LONG_KINDS[j % 6]``: (a) continuous values of both signs;
    (b) multiples of 0.25 in -0.5 .. 0.5 -- five values, so a 1024-entry column holds about 200 equal keys at every rank;
    (c) all equal; (d) continuous with NaN on a seeded half of the days, another half in every column; (e) NaN throughout;
    (f) +0.0 and -0.0 mixed with denormals and the smallest normals of both signs.  Rows 1030.. are +inf."""
    rng = np.random.default_rng(1000 * n + seed)
    dtype = np.dtype(dtype).type
    tiny, small = np.finfo(dtype).smallest_subnormal, np.finfo(dtype).tiny
    X = np.empty((LONG_T, n), dtype=dtype)
    for j in range(n):
        kind = LONG_KINDS[j % 6]
        if kind == "a":
            col = rng.uniform(-30.0, 45.0, LONG_T)
        elif kind == "b":
            col = 0.25 * rng.integers(-2, 3, LONG_T)
        elif kind == "c":
            col = np.full(LONG_T, 287.65)
        elif kind == "d":
            col = rng.uniform(-30.0, 45.0, LONG_T)
            col[rng.permutation(LONG_T)[:LONG_T // 2]] = np.nan
        elif kind == "e":
            col = np.full(LONG_T, np.nan)
        else:
            col = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, -2 * tiny, small, -small], dtype=dtype)[rng.integers(0, 8, LONG_T)]
        X[:, j] = col
    X[LONG_LISTED:] = np.inf
    return X


def long_season(n):
    """``(doy, windows)`` of the long shape: ``doy = 1 + (t % 366)`` and per cell one of the six kinds of window of
    tests/test_gpu_seasons.py (open all year, null, empty, a single day, a plain interval, a wrapping one), the kind stepping on by
    one every six cells so that every kind of window meets every kind of column of :func:`long_field`"""
    from tests.test_gpu_seasons import _mixed_cells, _pack
    doy = 1 + np.arange(LONG_T) % 366
    every = _pack(*_mixed_cells(6 * n, doy))                                     # entry i: kind i % 6
    pick = np.array([6 * j + (j + j // 6) % 6 for j in range(n)])
    return doy, np.ascontiguousarray(every[pick])


def valid_counts(X, row_begin, rows, doy=None, windows=None):
    """``m[p, j]``: the valid entries of period ``p`` for cell ``j`` (the definition's, counted without sorting anything)"""
    X = np.asarray(X)
    T, n = X.shape
    ok = ~np.isnan(X)
    if doy is not None:
        ok &= np.stack([in_season(int(d), windows) for d in doy])
    m = np.zeros((len(row_begin) - 1, n), dtype=np.int64)
    for p in range(len(row_begin) - 1):
        lst = np.asarray(rows[row_begin[p]:row_begin[p + 1]], dtype=np.int64)
        lst = lst[(lst >= 0) & (lst < T)]
        m[p] = ok[lst].sum(axis=0)
    return m
