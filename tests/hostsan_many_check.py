#!/usr/bin/env python3
"""Drives the many-plan builder (wagg_plan_create_many) of libwagg under AddressSanitizer + UBSan, as
tests/hostsan_check.py does for the single-plan builder.  Run through tests/test_many_host.py, which builds
`make -C climate_toolbox_amd/csrc hostsan` and preloads the sanitizer runtime; ctypes only (no torch).

Exit status 0 = every call returned what it should and the sanitizers stayed silent."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = C.CDLL(os.path.join(ROOT, "climate_toolbox_amd", "lib", "libwagg_hostsan.so"))
L.wagg_last_error.restype = C.c_char_p
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def create(ci, rc, ws, G, R, levels, row_len=720):
    wp = (f64p * max(1, len(ws)))(*[p(w, C.c_double) for w in ws])
    lp = (i32p * max(1, len(levels)))(*[p(c, C.c_int32) for c, _ in levels])
    lr = (C.c_int32 * max(1, len(levels)))(*[r for _, r in levels])
    h = C.c_void_p()
    st = L.wagg_plan_create_many(p(ci, C.c_int32), p(rc, C.c_int32), wp, len(ws), C.c_int64(len(ci)), C.c_int64(G), C.c_int32(R),
                                 C.c_int64(row_len), lp, lr, len(levels), 0, C.byref(h))
    if st == 0:
        L.wagg_plan_destroy(h)
    return st


rng = np.random.default_rng(0)
G, R = 720 * 90, 1500
for nseg in (0, 1, 40000):
    ci = rng.integers(0, G, nseg).astype(np.int32)
    rc = rng.integers(-1, R, nseg).astype(np.int32)
    iso = np.where(rc < 0, -1, rc // 10).astype(np.int32)
    cont = np.where(rc < 0, -1, rc // 300).astype(np.int32)
    ws = [rng.uniform(-0.1, 1, nseg) for _ in range(4)]
    ws[1][::11] = np.nan
    for k in (1, 2, 4):
        for levels in ([], [(iso, 150)], [(iso, 150), (cont, 5)]):
            st = create(ci, rc, ws[:k], G, R, levels)
            assert st in (0, -2, -4), (st, L.wagg_last_error())
    if nseg > 1:
        # a fine region with two rows: its last row moves to another coarse region (ws[0] keeps every row)
        vals, first, counts = np.unique(rc, return_index=True, return_counts=True)
        r2 = vals[(vals >= 0) & (counts >= 2)][0]
        last = np.nonzero(rc == r2)[0][-1]
        bad = iso.copy(); bad[last] = (bad[last] + 1) % 150
        assert create(ci, rc, ws[:2], G, R, [(bad, 150)]) == -1
        assert b"does not nest" in L.wagg_last_error()
        oob = iso.copy(); oob[3] = 150
        assert create(ci, rc, ws[:2], G, R, [(oob, 150)]) == -1
        assert create(ci, rc, ws[:4] + ws[:1], G, R, []) == -1
print("hostsan many ok")
