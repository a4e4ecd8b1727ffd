#!/usr/bin/env python3
"""Coefficients of Q in csrc/wagg_exposure.hip::exposure1<float>: the fraction of a day the sinusoid through (lo, hi) spends
above e is A = acos(z) / pi, z = (e - M) / w.  With t = 1 - |z| in [0, 1],  acos(1 - t) / pi = sqrt(t) Q(t)  and Q is smooth
between sqrt(2) / pi (t = 0) and 1 / 2 (t = 1); the other half follows from A(-z) = 1 - A(z).  Chebyshev fit of Q,
converted to monomials for the Horner form; prints the coefficients (high to low), the error of the fit in A, and the error
of the whole fp32 formula -- t from min(hi - e, e - lo) / w as the kernel forms it -- against the fp64 libm evaluation on
random fields and on days whose tasmax is a few ulps above the edge.

usage: fit_acos_poly.py [degree]      (default 6)"""
import sys

import numpy as np
from numpy.polynomial import chebyshev as C


def Q(t):
    out = np.empty_like(t)
    big = t > 1e-4
    out[big] = np.arccos(1 - t[big]) / np.pi / np.sqrt(t[big])
    ts = t[~big]      # series at t -> 0 (acos(1 - t) = sqrt(2 t) (1 + t / 12 + 3 t^2 / 160 + ...))
    out[~big] = np.sqrt(2.0) * (1 + ts / 12 + 3 * ts ** 2 / 160 + 5 * ts ** 3 / 896) / np.pi
    return out


deg = int(sys.argv[1]) if len(sys.argv) > 1 else 6
ts = (np.cos(np.pi * (np.arange(4000) + 0.5) / 4000) + 1) / 2
c = C.chebfit(2 * ts - 1, Q(ts), deg)
tt = np.linspace(0, 1, 400001)
print("degree %d: max |sqrt(t) (fit - Q)| on [0, 1] (the error in A): %.3g" % (deg, (np.sqrt(tt) * np.abs(C.chebval(2 * tt - 1, c) - Q(tt))).max()))
pu = C.cheb2poly(c)
px = np.zeros(1)
for k, a in enumerate(pu):
    term = np.array([1.0])
    for _ in range(k):
        term = np.convolve(term, [-1.0, 2.0])
    px = np.pad(px, (0, max(0, len(term) - len(px))))
    px[:len(term)] += a * term
f32 = np.float32
q32 = [f32(v) for v in px]
print("Horner coefficients, high to low:", [repr(float(v)) for v in q32[::-1]])


def formula32(lo, hi, e):
    """the kernel's band expression, every operation rounded to fp32"""
    with np.errstate(all="ignore"):
        rw = (f32(1) / (f32(0.5) * (hi - lo))).astype(f32)
        dlo, dhi = (e - lo).astype(f32), (hi - e).astype(f32)
        t = np.fmin(np.fmax((np.fmin(dlo, dhi) * rw).astype(f32), f32(0)), f32(1))
        p = np.full_like(t, q32[-1])
        for a in q32[-2::-1]:
            p = (p * t + a).astype(f32)
        s = (np.sqrt(t).astype(f32) * p).astype(f32)
        a = np.where(dhi <= dlo, s, (f32(1) - s).astype(f32))
        return np.fmin(np.fmax(a, f32(0)), f32(1))


def libm64(lo, hi, e):
    lo, hi, e = lo.astype(np.float64), hi.astype(np.float64), np.float64(e)
    with np.errstate(all="ignore"):
        return np.clip(np.arccos(np.clip((e - (hi + lo) / 2) / ((hi - lo) / 2), -1, 1)) / np.pi, 0, 1)


# the coefficients as rounded to fp32, evaluated in fp64: what the fit itself contributes
p = np.full_like(tt, float(q32[-1]))
for a in q32[-2::-1]:
    p = p * tt + float(a)
print("fp32-rounded coefficients: max error in A %.3g" % np.abs(np.sqrt(tt) * p - np.arccos(1 - tt) / np.pi).max())
rng = np.random.default_rng(0)
n = 2_000_000
lo = rng.uniform(-20, 40, n).astype(f32)
hi = (lo + rng.uniform(0.01, 20, n).astype(f32)).astype(f32)
e = (lo + (hi - lo) * rng.uniform(0.0, 1.0, n).astype(f32)).astype(f32)
e = np.where((lo < e) & (hi > e), e, (f32(0.5) * (lo + hi)).astype(f32))
err = np.abs(formula32(lo, hi, e) - libm64(lo, hi, e))
print("fp32 formula vs fp64 libm, random days in band: max abs error %.3g, mean %.3g" % (err.max(), err.mean()))
for ulps in (1, 2, 4, 16, 256):
    ee = rng.uniform(0, 40, 100000).astype(f32)
    hh = ee.copy()
    for _ in range(ulps):
        hh = np.nextafter(hh, f32(np.inf))
    ll = (ee - rng.uniform(1, 15, len(ee)).astype(f32)).astype(f32)
    err = np.abs(formula32(ll, hh, ee) - libm64(ll, hh, ee))
    print("tasmax %3d ulps above the edge: max abs error %.3g (A itself up to %.3g)" % (ulps, err.max(), libm64(ll, hh, ee).max()))
