"""The sinusoid exposure bins (wagg_exposure_reduce_*, include/wagg.h) restated in NumPy.  The shift ``x + offset`` and the
conversion of the edge are taken in the element type, as the kernel takes them; everything after that is fp64 with np.arccos:

    A(lo, hi, e) = 0                          if lo or hi is NaN      (checked first)
                 = 1                          if !(lo < e)
                 = 0                          if !(hi > e)
                 = clip(arccos(z) / pi, 0, 1) otherwise,  z = clip((e - M) / w, -1, 1),  M = (hi + lo) / 2,  w = (hi - lo) / 2

bin k of a day = A(e_k) - A(e_k+1); a period's bin = the sum over its listed rows on which the cell is in season."""
import numpy as np


def shifted(x, offset):
    """x + offset in x's own dtype, as float64"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x + x.dtype.type(offset)).astype(np.float64)


def edge_in(dtype, e):
    """the edge as the kernel sees it: converted to the element type (float64 of it)"""
    with np.errstate(over="ignore"):
        return np.float64(np.dtype(dtype).type(e))


def fraction_above(lo, hi, e):
    """A(lo, hi, e) for float64 arrays lo, hi (already shifted) and a float64 edge"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = np.clip((e - (hi + lo) / 2.0) / ((hi - lo) / 2.0), -1.0, 1.0)
        band = np.clip(np.arccos(z) / np.pi, 0.0, 1.0)
        a = np.where(~(lo < e), 1.0, np.where(~(hi > e), 0.0, band))
    return np.where(np.isnan(lo) | np.isnan(hi), 0.0, a)


def day_bins(tasmin, tasmax, offset, edges):
    """(n_bins,) + tasmin.shape: every day's share of each bin, fp64"""
    dt = np.asarray(tasmin).dtype
    lo, hi = shifted(tasmin, offset), shifted(tasmax, offset)
    A = [fraction_above(lo, hi, edge_in(dt, e)) for e in edges]
    return np.stack([A[k] - A[k + 1] for k in range(len(A) - 1)])


def period_sum(daily, row_begin, rows, mask=None):
    """(..., T, n) daily values summed over each period's row list (rows may repeat) where ``mask`` (T, n) is nonzero: (..., P, n)"""
    daily = np.asarray(daily, dtype=np.float64)
    if mask is not None:
        daily = np.where(np.asarray(mask) > 0, daily, 0.0)
    rows = np.asarray(rows, dtype=np.int64)
    out = np.zeros(daily.shape[:-2] + (len(row_begin) - 1, daily.shape[-1]))
    for p in range(len(row_begin) - 1):
        out[..., p, :] = daily[..., rows[row_begin[p]:row_begin[p + 1]], :].sum(axis=-2)
    return out


def exposure_bins(tasmin, tasmax, offset, edges, row_begin, rows, mask=None):
    """(n_bins, P, n): the restatement of engine.exposure_reduce"""
    return period_sum(day_bins(tasmin, tasmax, offset, edges), row_begin, rows, mask)


def counted_days(tasmin, tasmax, row_begin, rows, mask=None):
    """(P, n): D, the listed in-season days of a cell on which neither field is NaN"""
    ok = ~(np.isnan(np.asarray(tasmin)) | np.isnan(np.asarray(tasmax)))
    return period_sum(ok.astype(np.float64), row_begin, rows, mask)
