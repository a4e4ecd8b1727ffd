"""The spell statistics of wagg_spell_span_* (include/wagg.h: spells that run across period boundaries), restated in plain
NumPy straight from the definition: the running length r_i and the whole length l of every entry of the CHAIN are computed first
(one forward and one backward loop over the chain, vectorised over cells and thresholds), and the three statistics are read off
them per period.  Nothing is credited backwards.  Used by tests/test_spell_span_host.py and the GPU tests of the span mode."""
import numpy as np

from tests.spell_ref import in_season


def chain_of(row_begin, n_rows):
    """``(b, e)``: the clamped bounds of every period's list, as WAGG_ROWLIST_ROWS clamps them"""
    rb = np.asarray(row_begin, dtype=np.int64)
    b = np.clip(rb[:-1], 0, n_rows)
    e = np.maximum(np.clip(rb[1:], 0, n_rows), b)
    return b, e


def running_and_whole(X, row_begin, rows, offset, thresholds, side="above", doy=None, windows=None):
    """``(period_of, r, ell)`` over the chain's entries ``c = 0 .. N - 1`` (the periods' lists one after the other):
    ``period_of[c]`` the period whose list holds the entry, ``r[k, c, j]`` its running length (0 when cold), ``ell[k, c, j]`` the
    whole length of its run (0 when cold)."""
    X = np.asarray(X)
    T, n = X.shape
    thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    rows = np.asarray(rows, dtype=np.int64)
    assert side in ("above", "below") and (doy is None) == (windows is None)
    b, e = chain_of(row_begin, len(rows))
    index = np.concatenate([np.arange(b[p], e[p]) for p in range(len(b))] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    period_of = np.concatenate([np.full(e[p] - b[p], p) for p in range(len(b))] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    t_of = rows[index]
    N = len(index)
    hot = np.zeros((len(thr), N, n), dtype=bool)
    for c in range(N):
        t = int(t_of[c])
        if not 0 <= t < T:
            continue                                                             # a row outside the field is cold
        v = X[t].astype(np.float64) + np.float64(offset)                        # (the shift in fp64, of the exact value)
        with np.errstate(invalid="ignore"):
            h = v[None, :] < thr[:, None] if side == "below" else v[None, :] >= thr[:, None]
        h &= ~np.isnan(v)[None, :]
        if doy is not None:
            h &= in_season(int(doy[t]), windows)[None, :]
        hot[:, c] = h
    joins = np.zeros(N, dtype=bool)
    joins[1:] = t_of[1:] == t_of[:-1] + 1                                        # whatever boundary lies between the two
    r = np.zeros((len(thr), N, n), dtype=np.int64)
    for c in range(N):
        before = r[:, c - 1] if c > 0 and joins[c] else 0
        r[:, c] = np.where(hot[:, c], before + 1, 0)
    ell = np.zeros_like(r)
    for c in range(N - 1, -1, -1):
        goes_on = hot[:, c + 1] if c + 1 < N and joins[c + 1] else np.zeros((len(thr), n), dtype=bool)
        ell[:, c] = np.where(hot[:, c], np.where(goes_on, ell[:, c + 1] if c + 1 < N else 0, r[:, c]), 0)
    return period_of, r, ell


def stats_from(period_of, r, ell, P, min_length, stat):
    """the statistic per period, read off the running and whole lengths: ``out[k, p, j]`` as float64"""
    L = int(min_length)
    assert stat in ("days", "events", "longest") and L >= 1
    out = np.zeros((r.shape[0], P, r.shape[2]), dtype=np.int64)
    for p in range(P):
        mine = period_of == p
        if not mine.any():
            continue
        if stat == "days":
            out[:, p] = ((r[:, mine] > 0) & (ell[:, mine] >= L)).sum(axis=1)
        elif stat == "events":
            out[:, p] = (r[:, mine] == L).sum(axis=1)
        else:
            out[:, p] = r[:, mine].max(axis=1)
    return out.astype(np.float64)


def spell_span_ref(X, row_begin, rows, offset, thresholds, min_length=1, stat="days", side="above", doy=None, windows=None):
    """``out[k, p, j]`` as float64: "days" the hot entries of p's list whose run has ``ell >= min_length``; "events" the entries
    of p's list with ``r == min_length``; "longest" the greatest ``r`` over p's list (0 for an empty one)."""
    period_of, r, ell = running_and_whole(X, row_begin, rows, offset, thresholds, side, doy, windows)
    return stats_from(period_of, r, ell, len(row_begin) - 1, min_length, stat)
