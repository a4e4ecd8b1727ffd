"""The exported wagg_*apply*_f32/_f64 symbols against hand-filled wagg_apply descriptors of the same calls: identical bits,
for both element types and both plan kinds (csrc/wagg_desc.hip: every symbol fills a descriptor; csrc/wagg_entry.h: the typed
layer behind it).  What can go wrong in that layer is a wrong element type or a swapped or dropped argument, which the
smallest shapes show as long as no two arguments are equal: the round-6 synthetic table at 24 x 48 cells, T = 3,
ldx = G + 3, ldo = R + 5 (T + 5 for (region, time) results), out_pstride = T * ldo + 7, offset -273.15, powers 2..3, two
thresholds.  The result buffers start as a sentinel: what a call does not own keeps it, and T = 0 writes nothing."""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, SENT, OFFSET, THR = 3, -777.0, -273.15, (5.0, 12.5)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    torch.cuda.set_device(0)
    from climate_toolbox_amd import _lib, synth
    from climate_toolbox_amd.engine import DensePlan, ShardGroup, SparsePlan
    e = types.SimpleNamespace(torch=torch, lib=_lib, L=_lib.load())
    lat, lon, df = synth.realistic_segments(nlat=24, nlon=48, R=20, n_iso=4, seed=3, land_frac=0.2, string_labels=False)
    cell, code, w, uniq = synth.code_segments(df, lat, lon, "areawt", "hierid")
    e.G, e.R = len(lat) * len(lon), len(uniq)
    e.ldx, e.ldo = e.G + 3, e.R + 5
    e.pstride = T * e.ldo + 7
    e.sparse = SparsePlan(cell, code, w, e.G, e.R, row_len=len(lon))
    e.sparse2 = e.sparse.replica(0)
    e.dense, e.clone = {}, {}
    for dt in ("float32", "float64"):
        e.dense[dt] = DensePlan.from_segments(cell, code, w, e.G, e.R, dtype=dt, form="full")
        e.clone[dt] = e.dense[dt].replica(0)               # (built from a table: wagg_dense_clone, a second plan on the same device)
        assert e.clone[dt]._h.value != e.dense[dt]._h.value
    e.group = ShardGroup([0, 0], transport="peer")
    rng = np.random.default_rng(6)
    e.x = {}
    for dt in ("float32", "float64"):
        mid = (280 + 10 * rng.standard_normal((T, e.ldx))).astype(dt)          # (the row padding holds data too: never read)
        e.x[dt] = types.SimpleNamespace(mid=mid, lo=mid - 5, hi=mid + 5, gt=np.ascontiguousarray(np.pad(mid[:, :e.G].T, ((0, 0), (0, 3)))))
    yield e
    e.group.close()
    for p in list(e.dense.values()) + list(e.clone.values()) + [e.sparse, e.sparse2]:
        p.close()


def _elem(e, dt):
    return e.lib.T_F32 if dt == "float32" else e.lib.T_F64


def _written(n, planes, rows, cols, ld, pstride):
    m = np.zeros(n, dtype=bool)
    for p in range(planes):
        for r in range(rows):
            m[p * pstride + r * ld: p * pstride + r * ld + cols] = True
    return m


def _same_call(e, dt, symbol, args, desc, host, n, written, inputs):
    """symbol(*args(out)) and wagg_apply(desc(out)) into two sentinel buffers of n elements: rc 0, the same bits everywhere,
    the sentinel kept outside `written` and gone inside it.  `inputs` are kept alive (and on the device for device calls)."""
    torch, L = e.torch, e.L
    outs = []
    for use_desc in (False, True):
        buf = np.full(n, SENT, dtype=dt)
        dev = None if host else torch.from_numpy(buf).cuda()
        ptr = buf.ctypes.data if host else dev.data_ptr()
        torch.cuda.synchronize()
        if use_desc:
            d = e.lib.ApplyDesc(struct_size=C.sizeof(e.lib.ApplyDesc), elem=_elem(e, dt), pow_first=1, n_pow=1)
            for k, v in desc(ptr).items():
                setattr(d, k, e.lib._ptr(v) if k in e.lib._DESC_POINTERS else v)
            rc = L.wagg_apply(C.byref(d))
        else:
            rc = getattr(L, "%s_%s" % (symbol, "f32" if dt == "float32" else "f64"))(*args(ptr))
        assert rc == 0, (symbol, dt, use_desc, L.wagg_last_error())
        torch.cuda.synchronize()
        outs.append(buf if host else dev.cpu().numpy())
    a, b = outs
    assert a.tobytes() == b.tobytes(), (symbol, dt)
    assert np.all(a[~written] == SENT) and np.all(a[written] != SENT) and np.all(np.isfinite(a)), (symbol, dt)
    del inputs
    return a


def _dev(e, *arrays):
    return [e.torch.from_numpy(a).cuda() for a in arrays]


DTYPES = ["float32", "float64"]


@pytest.mark.parametrize("dt", DTYPES)
def test_segment_table_plan_device(env, dt):
    e, x, lib = env, env.x[dt], env.lib
    h, vp = e.sparse._h, C.c_void_p
    X, lo, hi, Xgt = _dev(e, x.mid, x.lo, x.hi, x.gt)
    thr = (C.c_double * 2)(*THR)
    for layout, out_layout, Xl, ldx in ((lib.LAYOUT_TG, lib.OUT_TR, X, e.ldx), (lib.LAYOUT_GT, lib.OUT_RT, Xgt, T + 3),
                                        (lib.LAYOUT_TG, lib.OUT_RT, X, e.ldx)):
        rows, cols = (T, e.R) if out_layout == lib.OUT_TR else (e.R, T)
        ldo = cols + 5
        ps = rows * ldo + 7
        common = dict(plan_kind=lib.PLAN_SEGMENT, source=lib.SRC_DEVICE, plan=h, x=Xl.data_ptr(), ldx=ldx, ldo=ldo, layout=layout,
                      out_layout=out_layout)
        for Tn in (T, 0):
            w1 = _written(2 * ps, 1 if Tn else 0, rows, cols, ldo, ps)
            w2 = _written(2 * ps, 2 if Tn else 0, rows, cols, ldo, ps)
            _same_call(e, dt, "wagg_apply", lambda o: (h, vp(Xl.data_ptr()), Tn, ldx, layout, vp(o), ldo, out_layout, None),
                       lambda o: dict(common, T=Tn, out=o), False, 2 * ps, w1, Xl)
            _same_call(e, dt, "wagg_apply_poly",
                       lambda o: (h, vp(Xl.data_ptr()), Tn, ldx, layout, OFFSET, 2, 2, vp(o), ldo, ps, out_layout, None),
                       lambda o: dict(common, T=Tn, out=o, transform=lib.XF_POLY, offset=OFFSET, pow_first=2, n_pow=2, out_pstride=ps),
                       False, 2 * ps, w2, Xl)
            if layout == lib.LAYOUT_TG:
                _same_call(e, dt, "wagg_apply_edd",
                           lambda o: (h, vp(lo.data_ptr()), vp(hi.data_ptr()), Tn, ldx, layout, OFFSET, thr, 2, vp(o), ldo, ps, out_layout, None),
                           lambda o: dict(common, T=Tn, out=o, x=lo.data_ptr(), x2=hi.data_ptr(), transform=lib.XF_EDD, offset=OFFSET,
                                          thresholds=thr, n_thr=2, out_pstride=ps), False, 2 * ps, w2, (lo, hi))


@pytest.mark.parametrize("dt", DTYPES)
def test_segment_table_plan_host(env, dt):
    e, x, lib = env, env.x[dt], env.lib
    h, vp = e.sparse._h, C.c_void_p
    thr = (C.c_double * 2)(*THR)
    n, ps = 2 * e.pstride + e.R * (T + 5), e.pstride           # (two (T, R) planes, or one (R, T) result at ldo = T + 5)
    seg = dict(plan_kind=lib.PLAN_SEGMENT, plan=h, ldx=e.ldx, ldo=e.ldo)
    plain = None
    for Tn in (T, 0):
        w1, w2 = (_written(n, k if Tn else 0, T, e.R, e.ldo, ps) for k in (1, 2))
        for flags in (lib.HOST_PIN, lib.HOST_PIN | lib.HOST_WHOLE, lib.HOST_PIN | lib.HOST_LINES):
            got = _same_call(e, dt, "wagg_apply_host_ex",
                             lambda o: (h, vp(x.mid.ctypes.data), Tn, e.ldx, lib.LAYOUT_TG, vp(o), e.ldo, lib.OUT_TR, flags),
                             lambda o: dict(seg, source=lib.SRC_HOST, x=x.mid.ctypes.data, T=Tn, out=o, flags=flags), True, n, w1, x)
            if Tn and flags == lib.HOST_PIN | lib.HOST_LINES:
                plain = got
        # the plain symbol is _ex with HOST_PIN | HOST_LINES
        got = _same_call(e, dt, "wagg_apply_host", lambda o: (h, vp(x.mid.ctypes.data), Tn, e.ldx, lib.LAYOUT_TG, vp(o), e.ldo, lib.OUT_TR),
                         lambda o: dict(seg, source=lib.SRC_HOST, x=x.mid.ctypes.data, T=Tn, out=o, flags=lib.HOST_PIN | lib.HOST_LINES),
                         True, n, w1, x)
        if Tn:
            assert got.tobytes() == plain.tobytes()
        # a (gridcell, time) field: the whole-field fallback
        if Tn:
            wrt = _written(n, 1, e.R, T, T + 5, ps)
            _same_call(e, dt, "wagg_apply_host_ex",
                       lambda o: (h, vp(x.gt.ctypes.data), Tn, T + 3, lib.LAYOUT_GT, vp(o), T + 5, lib.OUT_RT, lib.HOST_PIN),
                       lambda o: dict(seg, source=lib.SRC_HOST, x=x.gt.ctypes.data, T=Tn, ldx=T + 3, ldo=T + 5, layout=lib.LAYOUT_GT,
                                      out_layout=lib.OUT_RT, out=o, flags=lib.HOST_PIN), True, n, wrt, x)
        hs, devs = (C.c_void_p * 2)(h, e.sparse2._h), (C.c_int32 * 2)(0, 0)
        _same_call(e, dt, "wagg_apply_host_multi", lambda o: (hs, devs, 2, vp(x.mid.ctypes.data), Tn, e.ldx, vp(o), e.ldo, lib.HOST_PIN),
                   lambda o: dict(seg, source=lib.SRC_HOST_MULTI, plan=hs, devices=devs, n_plans=2, x=x.mid.ctypes.data, T=Tn, out=o,
                                  flags=lib.HOST_PIN), True, n, w1, x)
        _same_call(e, dt, "wagg_apply_poly_host", lambda o: (h, vp(x.mid.ctypes.data), Tn, e.ldx, OFFSET, 2, 2, vp(o), e.ldo, ps, lib.HOST_PIN),
                   lambda o: dict(seg, source=lib.SRC_HOST, x=x.mid.ctypes.data, T=Tn, out=o, transform=lib.XF_POLY, offset=OFFSET,
                                  pow_first=2, n_pow=2, out_pstride=ps, flags=lib.HOST_PIN), True, n, w2, x)
        _same_call(e, dt, "wagg_apply_edd_host",
                   lambda o: (h, vp(x.lo.ctypes.data), vp(x.hi.ctypes.data), Tn, e.ldx, OFFSET, thr, 2, vp(o), e.ldo, ps, lib.HOST_PIN),
                   lambda o: dict(seg, source=lib.SRC_HOST, x=x.lo.ctypes.data, x2=x.hi.ctypes.data, T=Tn, out=o, transform=lib.XF_EDD,
                                  offset=OFFSET, thresholds=thr, n_thr=2, out_pstride=ps, flags=lib.HOST_PIN), True, n, w2, x)


@pytest.mark.parametrize("dt", DTYPES)
def test_dense_family_plan(env, dt):
    e, x, lib = env, env.x[dt], env.lib
    h, h2, vp = e.dense[dt]._h, e.clone[dt]._h, C.c_void_p
    X, lo, hi = _dev(e, x.mid, x.lo, x.hi)
    n = T * e.ldo + 7
    den = dict(plan_kind=lib.PLAN_DENSE, plan=h, ldx=e.ldx, ldo=e.ldo)
    thr = (C.c_double * 1)(THR[0])
    for Tn in (T, 0):
        w = _written(n, 1 if Tn else 0, T, e.R, e.ldo, 0)
        _same_call(e, dt, "wagg_dense_apply", lambda o: (h, vp(X.data_ptr()), Tn, e.ldx, vp(o), e.ldo, 0, None),
                   lambda o: dict(den, source=lib.SRC_DEVICE, x=X.data_ptr(), T=Tn, out=o), False, n, w, X)
        _same_call(e, dt, "wagg_dense_apply_poly", lambda o: (h, vp(X.data_ptr()), Tn, e.ldx, OFFSET, 2, vp(o), e.ldo, 0, None),
                   lambda o: dict(den, source=lib.SRC_DEVICE, x=X.data_ptr(), T=Tn, out=o, transform=lib.XF_POLY, offset=OFFSET, pow_first=2,
                                  n_pow=1), False, n, w, X)
        _same_call(e, dt, "wagg_dense_apply_edd",
                   lambda o: (h, vp(lo.data_ptr()), vp(hi.data_ptr()), Tn, e.ldx, OFFSET, THR[0], vp(o), e.ldo, 0, None),
                   lambda o: dict(den, source=lib.SRC_DEVICE, x=lo.data_ptr(), x2=hi.data_ptr(), T=Tn, out=o, transform=lib.XF_EDD,
                                  offset=OFFSET, thresholds=thr, n_thr=1), False, n, w, (lo, hi))
        for flags in (lib.HOST_PIN, lib.HOST_PIN | lib.HOST_WHOLE):
            _same_call(e, dt, "wagg_dense_apply_host", lambda o: (h, vp(x.mid.ctypes.data), Tn, e.ldx, vp(o), e.ldo, flags),
                       lambda o: dict(den, source=lib.SRC_HOST, x=x.mid.ctypes.data, T=Tn, out=o, flags=flags), True, n, w, x)
        hs, devs = (C.c_void_p * 2)(h, h2), (C.c_int32 * 2)(0, 0)
        _same_call(e, dt, "wagg_dense_apply_host_multi", lambda o: (hs, devs, 2, vp(x.mid.ctypes.data), Tn, e.ldx, vp(o), e.ldo, lib.HOST_PIN),
                   lambda o: dict(den, source=lib.SRC_HOST_MULTI, plan=hs, devices=devs, n_plans=2, x=x.mid.ctypes.data, T=Tn, out=o,
                                  flags=lib.HOST_PIN), True, n, w, x)


@pytest.mark.parametrize("dt", DTYPES)
def test_sharded_forms_on_one_device(env, dt):
    """two shards of the T rows (2 + 1, then 0 + 0) on device 0 through a peer-copy group of the same device listed twice"""
    e, x, lib = env, env.x[dt], env.lib
    vp = C.c_void_p
    X, = _dev(e, x.mid)
    n = T * e.ldo + 7
    item = X.element_size()
    for symbol, kind, hs in (("wagg_apply_sharded", lib.PLAN_SEGMENT, (C.c_void_p * 2)(e.sparse._h, e.sparse._h)),
                             ("wagg_dense_apply_sharded", lib.PLAN_DENSE, (C.c_void_p * 2)(e.dense[dt]._h, e.clone[dt]._h))):
        for split in ((2, 1), (0, 0)):
            xs = (C.c_void_p * 2)(X.data_ptr(), X.data_ptr() + split[0] * e.ldx * item)
            rows = (C.c_int64 * 2)(*split)
            w = _written(n, 1 if sum(split) else 0, T, e.R, e.ldo, 0)
            _same_call(e, dt, symbol, lambda o: (e.group._h, hs, xs, rows, e.ldx, vp(o), e.ldo, 1),
                       lambda o: dict(plan_kind=kind, source=lib.SRC_SHARDED, group=e.group._h, plan=hs, n_plans=2, x=xs, rows=rows, ldx=e.ldx,
                                      out=o, ldo=e.ldo, root=1), False, n, w, X)
