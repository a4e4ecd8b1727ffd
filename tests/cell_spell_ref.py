"""The per-cell-threshold spell statistics of wagg_cell_spells_* (include/wagg.h), restated in plain NumPy: tests/spell_ref.py's
loop over the entries of a period's list with a (K, M, n) threshold array, the plane of every period, the NaN-threshold rule and
the two sequential fp64 sums.  Used by tests/test_cell_spell_host.py and the tests/test_gpu_cell_spell*.py files."""
import numpy as np

from tests.spell_ref import in_season


def cell_spell_ref(X, row_begin, rows, offset, thr, plane_of_period=None, min_length=1, stat="days", side="above", doy=None,
                   windows=None):
    """``out[k, p, j]`` as float64 (counts are whole numbers; the sums are the fp64 accumulators, which the caller casts to the
    element type as the kernel does on the store).  ``thr``: (K, M, n) or (K, n) of X's dtype.  Period ``p`` reads plane ``m =
    plane_of_period[p]`` (None: 0 for M == 1, p for M == P); an ``m`` outside [0, M) makes the period NaN in every plane.  Entry
    ``i`` is hot when ``t = rows[i]`` lies in [0, T), the cell is in season and ``float64(X[t, j]) >= float64(thr) - offset``
    (``"below"``: ``<``) -- the comparison rule of include/wagg.h, the difference formed once in fp64; NaN days are never hot.
    Counts as tests/spell_ref.py; ``"amount"`` adds ``float64(x) + offset`` per hot entry, ``"excess"`` ``(float64(x) + offset) -
    float64(thr)`` (``"below"``: the reverse), one entry at a time in list order.  A NaN threshold makes the cell NaN."""
    X = np.asarray(X)
    T, n = X.shape
    thr = np.asarray(thr)
    if thr.ndim == 2:
        thr = thr[:, None, :]
    K, M = thr.shape[:2]
    assert thr.shape[2] == n
    row_begin, rows = np.asarray(row_begin, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    P, L = len(row_begin) - 1, int(min_length)
    assert stat in ("days", "events", "longest", "amount", "excess") and side in ("above", "below") and L >= 1
    assert stat not in ("longest", "amount", "excess") or L == 1
    assert (doy is None) == (windows is None)
    if plane_of_period is None:
        assert M == 1 or M == P
        plane_of_period = np.zeros(P, dtype=np.int64) if M == 1 else np.arange(P)
    off = np.float64(offset)
    sums = stat in ("amount", "excess")
    out = np.zeros((K, P, n), dtype=np.float64)
    for p in range(P):
        m = int(plane_of_period[p])
        if not 0 <= m < M:
            out[:, p] = np.nan
            continue
        th = thr[:, m, :].astype(np.float64)                                     # (K, n)
        c = th - off                                                             # one fp64 subtraction
        run = np.zeros((K, n), dtype=np.int64)
        acc = np.zeros((K, n), dtype=np.float64)
        prev = None
        for i in range(row_begin[p], row_begin[p + 1]):
            t = int(rows[i])
            if prev is not None and t != prev + 1:                               # a gap in the row numbers ends every run
                run[:] = 0
            prev = t
            if 0 <= t < T:
                x = X[t].astype(np.float64)
                with np.errstate(invalid="ignore"):
                    hot = x[None, :] < c if side == "below" else x[None, :] >= c
                if doy is not None:
                    hot = hot & in_season(int(doy[t]), windows)[None, :]
            else:
                x = np.full(n, np.nan)
                hot = np.zeros((K, n), dtype=bool)
            run = np.where(hot, run + 1, 0)
            if stat == "days":
                acc += np.where(run == L, L, np.where(run > L, 1, 0))
            elif stat == "events":
                acc += run == L
            elif stat == "longest":
                acc = np.maximum(acc, run)
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    a = x + off                                                  # first rounding
                    term = a[None, :] if stat == "amount" else (th - a[None, :] if side == "below" else a[None, :] - th)
                    acc = np.where(hot, acc + np.where(hot, term, 0.0), acc)     # one sequential fp64 addition per hot entry
        out[:, p] = np.where(np.isnan(th), np.nan, acc)
    return out
