"""The spell statistics of wagg_spell_reduce_* (include/wagg.h), restated in plain NumPy: a Python loop over the entries of a
period's list, vectorised over cells and thresholds.  Used by tests/test_spell_host.py and tests/test_gpu_spell.py."""
import numpy as np

WIN_INVERT, WIN_NULL = 1 << 20, 1 << 21


def in_season(d, w):
    """is day-of-year ``d`` inside each packed window of ``w``?  (bits 0-9 first day, 10-19 last day, bit 20 invert, bit 21 null;
    a day outside 0..1023 is in no season)"""
    w = np.asarray(w, dtype=np.int64)
    a, b = w & 1023, (w >> 10) & 1023
    inside = (d >= a) & (d <= b)
    return ((w & WIN_NULL) == 0) & (0 <= d <= 1023) & (inside != ((w & WIN_INVERT) != 0))


def spell_ref(X, row_begin, rows, offset, thresholds, min_length=1, stat="days", side="above", doy=None, windows=None):
    """``out[k, p, j]`` as float64.  Entry ``i`` of period ``p``'s list is hot when ``t = rows[i]`` lies in ``[0, T)``, cell ``j`` is
    in season on ``doy[t]`` (when a season is given) and ``float64(X[t, j]) + offset >= thresholds[k]`` (``side="above"``) or
    ``< thresholds[k]`` (``"below"``); NaN is never hot.  A run is a maximal stretch of hot entries with ``rows[i + 1] == rows[i]
    + 1``; it ends with the period's list.  ``"days"``: hot entries in runs of at least ``min_length``; ``"events"``: such runs;
    ``"longest"``: the longest run."""
    X = np.asarray(X)
    T, n = X.shape
    thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    row_begin, rows = np.asarray(row_begin, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    P, L = len(row_begin) - 1, int(min_length)
    assert stat in ("days", "events", "longest") and side in ("above", "below") and L >= 1
    assert (doy is None) == (windows is None)
    out = np.zeros((len(thr), P, n), dtype=np.int64)

    def close(p, ended, run):
        """tally the runs that end here (``ended``), by the definition: whole runs, once they are over"""
        r = np.where(ended, run, 0)
        if stat == "days":
            out[:, p] += np.where(r >= L, r, 0)
        elif stat == "events":
            out[:, p] += (r >= L) & (r > 0)
        else:
            out[:, p] = np.maximum(out[:, p], r)

    everywhere = np.ones((len(thr), n), dtype=bool)
    for p in range(P):
        run = np.zeros((len(thr), n), dtype=np.int64)
        prev = None
        for i in range(row_begin[p], row_begin[p + 1]):
            t = int(rows[i])
            if prev is not None and t != prev + 1:                               # a gap in the row numbers ends every run
                close(p, everywhere, run)
                run[:] = 0
            prev = t
            if 0 <= t < T:
                v = X[t].astype(np.float64) + np.float64(offset)                # (the Kelvin shift in fp64, of the exact value)
                with np.errstate(invalid="ignore"):
                    hot = v[None, :] < thr[:, None] if side == "below" else v[None, :] >= thr[:, None]
                hot &= ~np.isnan(v)[None, :]
                if doy is not None:
                    hot &= in_season(int(doy[t]), windows)[None, :]
            else:
                hot = np.zeros((len(thr), n), dtype=bool)
            close(p, ~hot, run)
            run = np.where(hot, run + 1, 0)
        close(p, everywhere, run)                                                # the end of the list ends every run
    return out.astype(np.float64)
