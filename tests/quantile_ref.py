"""The period quantiles of wagg_quantile_select_* (include/wagg.h), restated in plain NumPy: a Python loop per period and cell,
``np.sort`` of the cell's valid raw elements and the arithmetic of the definition in ``np.float64``, one operation a line so that
nothing can be fused.  Used by tests/test_quantile_host.py and tests/test_gpu_quantile.py."""
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
