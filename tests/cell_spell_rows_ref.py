"""The plane-per-row spell statistics of wagg_row_cell_spells_* (include/wagg.h), restated in plain NumPy: tests/cell_spell_ref.py's
loop with the plane looked up per ENTRY (``plane_of_row[rows[i]]``), the comparison value formed per row, the excess against that
row's threshold, the sticky NaN rule over COUNTED entries and the out-of-range-plane rule.  Used by tests/test_calendar_day_host.py
and the tests/test_gpu_cell_spell_rows*.py files."""
import numpy as np

from tests.spell_ref import in_season


def cell_spell_rows_ref(X, row_begin, rows, offset, thr, plane_of_row, min_length=1, stat="days", side="above", doy=None, windows=None):
    """``out[k, p, j]`` as float64 (counts are whole numbers; the sums are the fp64 accumulators, which the caller casts to the
    element type as the kernel does on the store).  ``thr``: (K, M, n) or (K, n) of X's dtype; ``plane_of_row``: T indices.  Entry
    ``i`` of period ``p``, with ``t = rows[i]`` in [0, T), reads plane ``m = plane_of_row[t]``; it is hot when the cell is in season
    and ``float64(X[t, j]) >= float64(thr[k, m, j]) - offset`` (``"below"``: ``<``), the difference formed once in fp64.  A gap in
    the row numbers, a cold entry and the list's end end a run.  ``"amount"`` adds ``float64(x) + offset`` per hot entry,
    ``"excess"`` ``(float64(x) + offset) - float64(thr[k, m, j])`` (``"below"``: the reverse), one entry at a time in list order.
    A cell is NaN for level k in period p when a COUNTED entry (row in the field, cell in season) had a NaN threshold; an ``m``
    outside [0, M) on a listed row inside the field makes the whole period NaN."""
    X = np.asarray(X)
    T, n = X.shape
    thr = np.asarray(thr)
    if thr.ndim == 2:
        thr = thr[:, None, :]
    K, M = thr.shape[:2]
    assert thr.shape[2] == n and len(plane_of_row) == T
    row_begin, rows = np.asarray(row_begin, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    P, L = len(row_begin) - 1, int(min_length)
    assert stat in ("days", "events", "longest", "amount", "excess") and side in ("above", "below") and L >= 1
    assert stat not in ("longest", "amount", "excess") or L == 1
    assert (doy is None) == (windows is None)
    off = np.float64(offset)
    out = np.zeros((K, P, n), dtype=np.float64)
    for p in range(P):
        run = np.zeros((K, n), dtype=np.int64)
        acc = np.zeros((K, n), dtype=np.float64)
        nan_thr = np.zeros((K, n), dtype=bool)
        bad_plane = False
        prev = None
        for i in range(row_begin[p], row_begin[p + 1]):
            t = int(rows[i])
            if prev is not None and t != prev + 1:                               # a gap in the row numbers ends every run
                run[:] = 0
            prev = t
            hot = np.zeros((K, n), dtype=bool)
            term = np.zeros((K, n))
            if 0 <= t < T:
                m = int(plane_of_row[t])
                if not 0 <= m < M:
                    bad_plane = True
                else:
                    counted = np.ones(n, dtype=bool) if doy is None else in_season(int(doy[t]), windows)
                    th = thr[:, m, :].astype(np.float64)                         # (K, n)
                    nan_thr |= np.isnan(th) & counted[None, :]
                    x = X[t].astype(np.float64)
                    with np.errstate(invalid="ignore", over="ignore"):
                        c = th - off                                             # one fp64 subtraction, per row
                        hot = (x[None, :] < c if side == "below" else x[None, :] >= c) & counted[None, :]
                        a = x + off                                              # first rounding
                        term = np.broadcast_to(a, (K, n)) if stat == "amount" else (th - a[None, :] if side == "below" else a[None, :] - th)
            run = np.where(hot, run + 1, 0)
            if stat == "days":
                acc += np.where(run == L, L, np.where(run > L, 1, 0))
            elif stat == "events":
                acc += run == L
            elif stat == "longest":
                acc = np.maximum(acc, run)
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    acc = np.where(hot, acc + np.where(hot, term, 0.0), acc)     # one sequential fp64 addition per hot entry
        out[:, p] = np.nan if bad_plane else np.where(nan_thr, np.nan, acc)
    return out
