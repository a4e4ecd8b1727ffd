"""The rolling-window extremes of wagg_rolling_reduce_* (include/wagg.h), restated in plain NumPy: a Python loop over the entries
of a period's list, vectorised over cells; EVERY window is formed from scratch from its W entries (no ring, no running counter).
Used by tests/test_rolling_host.py and tests/test_gpu_rolling.py."""
import numpy as np

from tests.spell_ref import WIN_INVERT, WIN_NULL, in_season  # noqa: F401

ROLL_WINDOW_MAX, ROLL_MAX_WINDOWS = 16, 8


def rolling_ref(X, row_begin, rows, offset, lengths, stat="max", of="mean", doy=None, windows=None):
    """``out[k, p, j]`` in ``X``'s dtype.  Entry ``i`` of period ``p``'s list is valid for cell ``j`` when ``t = rows[i]`` lies in
    ``[0, T)``, the cell is in season on ``doy[t]`` (when a season is given) and ``X[t, j]`` is not NaN.  A window of ``W`` days
    ends at entry ``i`` when the entries ``i - W + 1 .. i`` lie in this period's list, ``rows[m + 1] == rows[m] + 1`` along them
    and all are valid for the cell; its sum is ``((x[i] + x[i-1]) + x[i-2]) + ...`` in float64, newest to oldest.  ``m`` starts
    at -inf (``stat="max"``; +inf for ``"min"``) and takes a window's sum where it is strictly greater (less), in list order.
    The result is ``m / W + offset`` (``of="mean"``) or ``m + W * offset`` (``"sum"``) rounded once to the dtype, and NaN where
    the period holds no valid window for the cell."""
    X = np.asarray(X)
    T, n = X.shape
    row_begin, rows = np.asarray(row_begin, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    lengths = [int(w) for w in np.atleast_1d(lengths)]
    assert stat in ("max", "min") and of in ("mean", "sum") and (doy is None) == (windows is None)
    assert all(1 <= w <= ROLL_WINDOW_MAX for w in lengths)
    P = len(row_begin) - 1
    out = np.empty((len(lengths), P, n), dtype=X.dtype)

    def valid(t):
        if not 0 <= t < T:
            return np.zeros(n, dtype=bool)
        ok = ~np.isnan(X[t])
        if doy is not None:
            ok &= in_season(int(doy[t]), windows)
        return ok

    for k, W in enumerate(lengths):
        for p in range(P):
            m = np.full(n, -np.inf if stat == "max" else np.inf)
            count = np.zeros(n, dtype=np.int64)
            for i in range(int(row_begin[p]) + W - 1, int(row_begin[p + 1])):
                ts = [int(rows[i - a]) for a in range(W)]                        # newest to oldest
                if any(ts[a] != ts[a + 1] + 1 for a in range(W - 1)):
                    continue                                                     # the row numbers do not ascend by one
                ok = np.ones(n, dtype=bool)
                for t in ts:
                    ok &= valid(t)
                if not ok.any():
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    s = X[ts[0]].astype(np.float64)
                    for t in ts[1:]:
                        s = s + X[t].astype(np.float64)
                    take = ok & ((s > m) if stat == "max" else (s < m))          # strict; a NaN sum (inf - inf) is never taken
                m = np.where(take, s, m)
                count += ok
            with np.errstate(invalid="ignore", over="ignore"):
                r = m / np.float64(W) + np.float64(offset) if of == "mean" else m + np.float64(W) * np.float64(offset)
                out[k, p] = np.where(count > 0, r, np.nan).astype(X.dtype)
    return out


def brute_force_max_mean(X, row_begin, rows, W):
    """max over explicitly enumerated windows of ``W`` consecutive rows of a NaN-free field without a season: ``np.max`` of the
    stacked window sums (``np.sum`` over the stack: only for values whose sums are exact), divided by W; NaN where none exists"""
    X = np.asarray(X, dtype=np.float64)
    P = len(row_begin) - 1
    out = np.full((P, X.shape[1]), np.nan)
    for p in range(P):
        lst = [int(t) for t in rows[row_begin[p]:row_begin[p + 1]]]
        sums = [X[lst[a:a + W]].sum(axis=0) for a in range(len(lst) - W + 1) if lst[a:a + W] == list(range(lst[a], lst[a] + W))]
        if sums:
            out[p] = np.max(np.stack(sums), axis=0) / W
    return out
