"""Device-side objects over the C-ABI (include/wagg.h).  torch supplies device memory and streams
only; every number is produced by the HIP kernels in climate_toolbox_amd/csrc/.

``stream=``: a call that takes it queues ALL its device work there -- the kernels, the zero-fill of a new status word, the
relayout of a non-contiguous operand -- whichever stream is torch's current one, and waits for no other stream.  Two kinds of
call do wait, and say so: those that take HOST integers and upload them (row lists, ``doy`` / ``windows``, the index of
:func:`take_axis`) do that with a blocking copy on torch's CURRENT stream, complete when the call returns; and ``status`` /
``saw_inf`` / :func:`any_less` synchronise ``stream`` itself.  The tensors a call allocates (results, status word, workspace)
are allocated with ``stream`` current, so they belong to that stream in torch's caching allocator like anything made under
``with torch.cuda.stream(stream)``: use them there, or order the other stream behind it AND tell the allocator
(``other.wait_stream(stream)``, ``result.record_stream(other)``).  tests/test_gpu_stream_order.py pins this per call."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import LAYOUT_GT, LAYOUT_TG, OUT_RT, OUT_TR, WaggError

_LAYOUTS = {"TG": LAYOUT_TG, "GT": LAYOUT_GT}
_OUTS = {"TR": OUT_TR, "RT": OUT_RT}


def require_gpu():
    L = _lib.load()
    if L.wagg_device_count() < 1:
        raise WaggError("no HIP device visible: the aggregation engine has no CPU fallback")
    import torch
    if not torch.cuda.is_available():
        raise WaggError("torch sees no GPU (needed for device buffers and streams)")
    return torch


class _on_device:
    """``with _on_device(d):`` -- device ``d`` is current inside (None: leave it as it is)."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        if self.device is not None:
            import torch
            self._ctx = torch.cuda.device(int(self.device))
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.device is not None:
            self._ctx.__exit__(*exc)
        return False


def _current_device():
    import torch
    return int(torch.cuda.current_device())


def _stream_handle(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _on_stream(stream):
    """``with _on_stream(s):`` -- ``s`` is torch's current stream inside (None: leave it as it is).  What torch allocates, fills
    or uploads for a call is done in there, so that it is ordered on the stream the library call runs on and comes from that
    stream's blocks of the caching allocator -- not from those of whichever stream the caller happens to have current, which
    work queued there may still be writing."""
    import torch
    return torch.cuda.stream(stream)


def _elem(dtype):
    """WAGG_T_F32 / WAGG_T_F64 of a torch or numpy dtype"""
    return _lib.T_F64 if str(dtype).endswith("float64") else _lib.T_F32


def _ld(t):
    """Leading dimension of a 2-D row-contiguous tensor: the row pitch; a single row carries an
    arbitrary stride(0), so its own length stands in."""
    return max(int(t.stride(0)), int(t.shape[1]), 1) if t.shape[0] > 1 else max(1, int(t.shape[1]))


def _np_ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _host_out(out, shape, dtype):
    """The result array of a host form: the caller's (C-contiguous, right shape and dtype -- e.g. a page-locked block,
    which the library then uses as it is) or a fresh one."""
    if out is None:
        return np.empty(shape, dtype=dtype)
    if not (isinstance(out, np.ndarray) and tuple(out.shape) == tuple(shape) and out.dtype == np.dtype(dtype) and out.flags.c_contiguous
            and out.flags.writeable):
        raise ValueError("out must be a writeable C-contiguous %s array of shape %s" % (np.dtype(dtype), tuple(shape)))
    return out


def _check_X(X, layout):
    import torch
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dim() == 2):
        raise TypeError("X must be a 2-D CUDA torch tensor")
    if X.dtype not in (torch.float32, torch.float64):
        raise TypeError("X must be float32 or float64, got %s" % X.dtype)
    if X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError("X rows must be contiguous (stride(1) == 1)")
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'TG' or 'GT'")
    return X


class SparsePlan:
    """Coded segment table -> device plan (wagg_plan_create).  Immutable after construction."""

    def __init__(self, cell_idx, region_code, w_eff, G, R, row_len=0, flags=0, device=None):
        require_gpu()
        L = _lib.load()
        self._args = (cell_idx, region_code, w_eff, G, R, row_len, flags)      # what a replica on another device is built from
        ci = np.ascontiguousarray(cell_idx, dtype=np.int32)
        rc = np.ascontiguousarray(region_code, dtype=np.int32)
        we = np.ascontiguousarray(w_eff, dtype=np.float64)
        if not (ci.shape == rc.shape == we.shape and ci.ndim == 1):
            raise ValueError("cell_idx, region_code, w_eff must be 1-D and of equal length")
        self._h = C.c_void_p()
        self._lease = threading.Lock()       # held by whoever is applying a cached plan (aggregations._plan_for)
        self.G, self.R = int(G), int(R)
        with _on_device(device):
            self.device = _current_device()
            _lib.check(L.wagg_plan_create(_np_ptr(ci, C.c_int32), _np_ptr(rc, C.c_int32),
                                          _np_ptr(we, C.c_double), len(ci), self.G, self.R,
                                          int(row_len), int(flags), C.byref(self._h)), "wagg_plan_create")
        info = _lib.PlanInfo()
        _lib.check(L.wagg_plan_get_info_sized(self._h, C.byref(info), C.sizeof(info)), "wagg_plan_get_info_sized")
        self.info = {k: getattr(info, k) for k, _ in _lib.PlanInfo._fields_}
        den = np.empty(self.R, dtype=np.float64)
        _lib.check(L.wagg_plan_get_den(self._h, _np_ptr(den, C.c_double)), "wagg_plan_get_den")
        self.den = den

    def close(self):
        for r in getattr(self, "_replicas", {}).values():
            r.close()
        if getattr(self, "_h", None) is not None and self._h.value and _lib is not None and _lib._lib is not None:
            _lib._lib.wagg_plan_destroy(self._h)     # (module globals may be gone at interpreter exit)
            self._h = C.c_void_p()

    __del__ = close

    def status(self, stream=None):
        """Synchronise the stream and raise if any apply on this plan failed on the device
        (``wagg_plan_status``)."""
        _lib.check(_lib.load().wagg_plan_status(self._h, _stream_handle(stream)), "wagg_plan_status")

    def compact_cells(self, dtype):
        """The grid cell behind every position of the plan's quads-only compact row for element type ``dtype`` (float32 /
        float64; ``wagg_plan_compact_cells``): an int32 array of ``Gq`` cells, quad ``i`` of the sorted distinct referenced quads
        at positions ``4i .. 4i + 3`` -- the columns of :func:`pack_rows`.  None when the plan has no such row for that type
        (region-shaped chunkings only, ``PLAN_NO_LINES``).  Cached; treat the array as read-only."""
        eb = 8 if "float64" in str(dtype) else 4          # (torch / numpy dtypes, their names, the numpy scalar types)
        cache = self.__dict__.setdefault("_compact_cells", {})
        if eb not in cache:
            L = _lib.load()
            gq = C.c_int64(0)
            _lib.check(L.wagg_plan_compact_info(self._h, eb, C.byref(gq)), "wagg_plan_compact_info")
            cells = None
            if gq.value > 0:
                cells = np.empty(gq.value, dtype=np.int32)
                _lib.check(L.wagg_plan_compact_cells(self._h, eb, _np_ptr(cells, C.c_int32)), "wagg_plan_compact_cells")
                cells.setflags(write=False)
            cache[eb] = cells
        return cache[eb]

    def apply(self, X, layout="TG", out=None, out_layout="TR", stream=None, compact=False):
        """out[t, r] on the device; asynchronous on torch's current stream (or `stream`: a new ``out`` then belongs to that stream in
        torch's allocator -- the module's docstring says what that asks of a caller who reads it on another).  ``compact=True``: the rows of X are
        PACKED rows (:func:`pack_rows`; at least ``len(compact_cells(X.dtype))`` columns, of which the first ``Gq`` are read)
        -- ``WAGG_APPLY_COMPACT_ROWS``: "TG" in, "TR" out only; the same bits as the plain apply of the unpacked rows."""
        import torch
        X = _check_X(X, layout)
        T = X.shape[0] if layout == "TG" else X.shape[1]
        n_g = X.shape[1] if layout == "TG" else X.shape[0]
        if compact:
            if layout != "TG" or out_layout != "TR":
                raise ValueError("compact rows are (time, cell) data and give a (time, region) result")
            cells = self.compact_cells(X.dtype)
            if cells is None:
                raise WaggError("this plan has no compact row for %s data" % (X.dtype,))
            if n_g < len(cells):
                raise ValueError("X has %d columns, a packed row of this plan %d" % (n_g, len(cells)))
        elif n_g != self.G:
            raise ValueError("X has %d grid cells, plan expects %d" % (n_g, self.G))
        shape = (T, self.R) if out_layout == "TR" else (self.R, T)
        if out is None:
            with _on_stream(stream):
                out = torch.empty(shape, dtype=X.dtype, device=X.device)
        elif tuple(out.shape) != shape or out.dtype != X.dtype or (shape[1] > 1 and out.stride(1) != 1):
            raise ValueError("out must be a %s %s tensor with contiguous rows" % (shape, X.dtype))
        _lib.run("wagg_apply", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(X.dtype), source=_lib.SRC_DEVICE,
                 x=X.data_ptr(), T=T, ldx=_ld(X), layout=_LAYOUTS[layout], out=out.data_ptr(), ldo=_ld(out),
                 out_layout=_OUTS[out_layout], stream=_stream_handle(stream), flags=_lib.APPLY_COMPACT_ROWS if compact else 0)
        return out

    def apply_poly(self, X, offset, n_pow, layout="TG", out=None, out_layout="TR", stream=None, pow_first=1):
        """out[i, t, r] = aggregate of (X + offset)**(pow_first + i), i < n_pow (``wagg_apply_poly_*``:
        the arithmetic of tas_poly, transformations.py:188, fused into the loads of the aggregation)."""
        import torch
        X = _check_X(X, layout)
        T = X.shape[0] if layout == "TG" else X.shape[1]
        n_g = X.shape[1] if layout == "TG" else X.shape[0]
        if n_g != self.G:
            raise ValueError("X has %d grid cells, plan expects %d" % (n_g, self.G))
        shape = (int(n_pow),) + ((T, self.R) if out_layout == "TR" else (self.R, T))
        if out is None:
            with _on_stream(stream):
                out = torch.empty(shape, dtype=X.dtype, device=X.device)
        elif tuple(out.shape) != shape or out.dtype != X.dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s %s tensor" % (shape, X.dtype))
        _lib.run("wagg_apply (poly)", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(X.dtype), source=_lib.SRC_DEVICE,
                 transform=_lib.XF_POLY, offset=float(offset), pow_first=int(pow_first), n_pow=int(n_pow),
                 x=X.data_ptr(), T=T, ldx=_ld(X), layout=_LAYOUTS[layout], out=out.data_ptr(), ldo=max(1, shape[2]),
                 out_pstride=shape[1] * shape[2], out_layout=_OUTS[out_layout], stream=_stream_handle(stream))
        return out

    def apply_edd(self, tasmin, tasmax, thresholds, offset=0.0, layout="TG", out=None, out_layout="TR", stream=None):
        """out[i, t, r] = aggregate of snyder_edd(tasmin + offset, tasmax + offset, thresholds[i])
        (``wagg_apply_edd_*``; transformations.py:7-93 evaluated while the two fields are loaded)."""
        import torch
        tasmin, tasmax = _check_X(tasmin, layout), _check_X(tasmax, layout)
        if tasmin.shape != tasmax.shape or tasmin.dtype != tasmax.dtype or _ld(tasmin) != _ld(tasmax):
            raise ValueError("tasmin and tasmax must have the same shape, dtype and row stride")
        T = tasmin.shape[0] if layout == "TG" else tasmin.shape[1]
        n_g = tasmin.shape[1] if layout == "TG" else tasmin.shape[0]
        if n_g != self.G:
            raise ValueError("fields have %d grid cells, plan expects %d" % (n_g, self.G))
        thr = np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
        shape = (len(thr),) + ((T, self.R) if out_layout == "TR" else (self.R, T))
        if out is None:
            with _on_stream(stream):
                out = torch.empty(shape, dtype=tasmin.dtype, device=tasmin.device)
        elif tuple(out.shape) != shape or out.dtype != tasmin.dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s %s tensor" % (shape, tasmin.dtype))
        _lib.run("wagg_apply (edd)", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(tasmin.dtype), source=_lib.SRC_DEVICE,
                 transform=_lib.XF_EDD, offset=float(offset), thresholds=thr.ctypes.data, n_thr=len(thr),
                 x=tasmin.data_ptr(), x2=tasmax.data_ptr(), T=T, ldx=_ld(tasmin), layout=_LAYOUTS[layout], out=out.data_ptr(),
                 ldo=max(1, shape[2]), out_pstride=shape[1] * shape[2], out_layout=_OUTS[out_layout], stream=_stream_handle(stream))
        return out

    def replica(self, device):
        """The same table as a plan on another device (multi-device host streaming)."""
        return SparsePlan(*self._args, device=device)

    def apply_host(self, X, layout="TG", out_layout="TR", flags=0, replicas=(), out=None):
        """Blocking host-buffer form (wagg_apply_host_ex_*): numpy in, numpy out.  (time, gridcell) data
        is streamed through the device in row blocks (H2D of block i+1, the kernels of block i and the
        return of block i-1 at once); ``flags``: ``_lib.HOST_PIN`` page-locks the arrays for the call,
        ``_lib.HOST_WHOLE`` copies the whole field at once, ``_lib.HOST_LINES`` lets host threads pack the 128-byte
        lines the table references so that only those cross PCIe (one device; ignored with ``replicas``).  ``replicas``: further plans of the same table
        on other devices (``replica(d)``): the row blocks are then dealt over all of them
        (``wagg_apply_host_multi_*``), each device on its own PCIe link."""
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64) or X.ndim != 2:
            raise TypeError("X must be a 2-D float32/float64 array")
        T = X.shape[0] if layout == "TG" else X.shape[1]
        shape = (T, self.R) if out_layout == "TR" else (self.R, T)
        out = _host_out(out, shape, X.dtype)
        if replicas:
            if layout != "TG" or out_layout != "TR":
                raise ValueError("the multi-device form takes (time, gridcell) data only")
            plans = (self,) + tuple(replicas)
            hs = (C.c_void_p * len(plans))(*[p._h for p in plans])
            devs = (C.c_int32 * len(plans))(*[p.device for p in plans])
            _lib.run("wagg_apply (host, multi-device)", plan_kind=_lib.PLAN_SEGMENT, plan=hs, n_plans=len(plans), devices=devs,
                     elem=_elem(X.dtype), source=_lib.SRC_HOST_MULTI, x=X.ctypes.data, T=T, ldx=X.shape[1], out=out.ctypes.data,
                     ldo=max(1, self.R), flags=int(flags) & ~(_lib.HOST_LINES | _lib.HOST_LINES_WHOLE))
            return out
        with _on_device(self.device):
            _lib.run("wagg_apply (host)", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(X.dtype), source=_lib.SRC_HOST,
                     x=X.ctypes.data, T=T, ldx=X.shape[1], layout=_LAYOUTS[layout], out=out.ctypes.data, ldo=max(1, shape[1]),
                     out_layout=_OUTS[out_layout], flags=int(flags))
        return out


    def apply_poly_host(self, X, offset, n_pow, pow_first=1, flags=0, out=None):
        """The fused powers of a host-resident (time, gridcell) field (``wagg_apply_poly_host_*``): numpy in, a
        (n_pow, T, R) numpy array out; the field crosses PCIe once (``_lib.HOST_LINES``: only the lines the table
        references), every row block is raised to its powers on the device."""
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64) or X.ndim != 2:
            raise TypeError("X must be a 2-D float32/float64 array")
        if X.shape[1] != self.G:
            raise ValueError("X has %d grid cells, plan expects %d" % (X.shape[1], self.G))
        T = X.shape[0]
        out = _host_out(out, (int(n_pow), T, self.R), X.dtype)
        with _on_device(self.device):
            _lib.run("wagg_apply (host, poly)", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(X.dtype), source=_lib.SRC_HOST,
                     transform=_lib.XF_POLY, offset=float(offset), pow_first=int(pow_first), n_pow=int(n_pow), x=X.ctypes.data, T=T,
                     ldx=X.shape[1], out=out.ctypes.data, ldo=max(1, self.R), out_pstride=max(1, T * self.R), flags=int(flags))
        return out


    def apply_edd_host(self, tasmin, tasmax, thresholds, offset=0.0, flags=0, out=None):
        """Snyder degree days of two host-resident (time, gridcell) fields at each threshold, aggregated
        (``wagg_apply_edd_host_*``): numpy in, a (n_thr, T, R) numpy array out; both fields cross PCIe once
        (``_lib.HOST_LINES``: only the lines the table references), the formula runs on the device."""
        tasmin, tasmax = np.ascontiguousarray(tasmin), np.ascontiguousarray(tasmax)
        if tasmin.dtype not in (np.float32, np.float64) or tasmin.ndim != 2:
            raise TypeError("fields must be 2-D float32/float64 arrays")
        if tasmin.shape != tasmax.shape or tasmin.dtype != tasmax.dtype:
            raise ValueError("tasmin and tasmax must have the same shape and dtype")
        if tasmin.shape[1] != self.G:
            raise ValueError("fields have %d grid cells, plan expects %d" % (tasmin.shape[1], self.G))
        thr = np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
        T = tasmin.shape[0]
        out = _host_out(out, (len(thr), T, self.R), tasmin.dtype)
        with _on_device(self.device):
            _lib.run("wagg_apply (host, edd)", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(tasmin.dtype), source=_lib.SRC_HOST,
                     transform=_lib.XF_EDD, offset=float(offset), thresholds=thr.ctypes.data, n_thr=len(thr), x=tasmin.ctypes.data,
                     x2=tasmax.ctypes.data, T=T, ldx=tasmin.shape[1], out=out.ctypes.data, ldo=max(1, self.R),
                     out_pstride=max(1, T * self.R), flags=int(flags))
        return out


def _many_args(cell_idx, region_code, w_effs, levels):
    """ctypes arguments of wagg_plan_create_many (and the arrays behind them, which the caller keeps alive for the call)."""
    ci = np.ascontiguousarray(cell_idx, dtype=np.int32)
    rc = np.ascontiguousarray(region_code, dtype=np.int32)
    ws = [np.ascontiguousarray(w, dtype=np.float64) for w in w_effs]
    lcs = [np.ascontiguousarray(c, dtype=np.int32) for c, _ in levels]
    if not (ci.ndim == 1 and ci.shape == rc.shape and all(a.shape == ci.shape for a in ws + lcs)):
        raise ValueError("cell_idx, region_code, every weight column and every level column must be 1-D and of equal length")
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    wp = (f64p * max(1, len(ws)))(*[_np_ptr(w, C.c_double) for w in ws])
    lp = (i32p * max(1, len(lcs)))(*[_np_ptr(c, C.c_int32) for c in lcs])
    lr = (C.c_int32 * max(1, len(levels)))(*[int(r) for _, r in levels])
    keep = (ci, rc, ws, lcs, wp, lp, lr)
    return keep, (_np_ptr(ci, C.c_int32), _np_ptr(rc, C.c_int32), wp, len(ws), len(ci)), (lp, lr, len(levels))


class ManyPlan:
    """K weightings x (the fine level + nested coarse levels) of one coded segment table (``wagg_plan_create_many``).
    ``w_effs``: K backup-filled weight columns (K <= 4); ``levels``: up to three ``(coarse_code, R_coarse)`` pairs, each
    code column nesting in ``region_code`` (-1 = null).  One apply reads X once (one PCIe crossing for a host-resident
    field) and returns views ``[level][weighting]`` into ONE result whose region axis concatenates every plane
    (level-major, then weighting; level 0 is the fine one)."""

    def __init__(self, cell_idx, region_code, w_effs, G, R, row_len=0, levels=(), flags=0, device=None):
        require_gpu()
        L = _lib.load()
        levels = [(c, int(r)) for c, r in levels]
        keep, head, tail = _many_args(cell_idx, region_code, w_effs, levels)
        self._h = C.c_void_p()
        self._lease = threading.Lock()       # held by whoever is applying a cached plan (_plans.py)
        self.G, self.R = int(G), int(R)
        with _on_device(device):
            self.device = _current_device()
            _lib.check(L.wagg_plan_create_many(*head, self.G, self.R, int(row_len), tail[0], tail[1], tail[2], int(flags),
                                               C.byref(self._h)), "wagg_plan_create_many")
        del keep
        k, nl, oc = C.c_int(0), C.c_int(0), C.c_int64(0)
        lr = (C.c_int32 * 4)()
        _lib.check(L.wagg_plan_many_info(self._h, C.byref(k), C.byref(nl), lr, C.byref(oc)), "wagg_plan_many_info")
        self.n_weights, self.n_levels, self.out_cols = k.value, nl.value, int(oc.value)
        self.level_R = [self.R] + [int(lr[i]) for i in range(self.n_levels)]
        self.offsets = []                    # offsets[l][k]: first column of plane (l, k)
        off = 0
        for Rl in self.level_R:
            self.offsets.append([off + i * Rl for i in range(self.n_weights)])
            off += self.n_weights * Rl
        info = _lib.PlanInfo()
        _lib.check(L.wagg_plan_get_info_sized(self._h, C.byref(info), C.sizeof(info)), "wagg_plan_get_info_sized")
        self.info = {k: getattr(info, k) for k, _ in _lib.PlanInfo._fields_}   # the fine level's chunkings; R = out_cols
        self.info["nnz"] *= self.n_weights                                       # (device bytes: one segment table per weighting)
        self.den = []
        for lv, Rl in enumerate(self.level_R):
            row = []
            for i in range(self.n_weights):
                d = np.empty(Rl, dtype=np.float64)
                _lib.check(L.wagg_plan_get_den_many(self._h, i, lv, _np_ptr(d, C.c_double)), "wagg_plan_get_den_many")
                row.append(d)
            self.den.append(row)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and _lib is not None and _lib._lib is not None:
            _lib._lib.wagg_plan_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def status(self, stream=None):
        """Synchronise the stream and raise if an apply on this plan failed on the device (``wagg_plan_status``)."""
        _lib.check(_lib.load().wagg_plan_status(self._h, _stream_handle(stream)), "wagg_plan_status")

    def split(self, full, out_layout="TR"):
        """Views [level][weighting] of a concatenated result."""
        if out_layout == "TR":
            return [[full[:, o:o + Rl] for o in offs] for offs, Rl in zip(self.offsets, self.level_R)]
        return [[full[o:o + Rl] for o in offs] for offs, Rl in zip(self.offsets, self.level_R)]

    def apply(self, X, layout="TG", out_layout="TR", out=None, stream=None):
        """Every plane from one pass over the device tensor X; asynchronous on torch's current stream (or `stream`: a new ``out``
        then belongs to that stream in torch's allocator, see the module's docstring).
        ``out``: the concatenated (T, out_cols) / (out_cols, T) result to fill (else a new one)."""
        import torch
        X = _check_X(X, layout)
        T = X.shape[0] if layout == "TG" else X.shape[1]
        if (X.shape[1] if layout == "TG" else X.shape[0]) != self.G:
            raise ValueError("X has the wrong number of grid cells (plan expects %d)" % self.G)
        shape = (T, self.out_cols) if out_layout == "TR" else (self.out_cols, T)
        if out is None:
            with _on_stream(stream):
                out = torch.empty(shape, dtype=X.dtype, device=X.device)
        elif tuple(out.shape) != shape or out.dtype != X.dtype or (shape[1] > 1 and out.stride(1) != 1):
            raise ValueError("out must be a %s %s tensor with contiguous rows" % (shape, X.dtype))
        _lib.run("wagg_apply (many)", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(X.dtype), source=_lib.SRC_DEVICE,
                 x=X.data_ptr(), T=T, ldx=_ld(X), layout=_LAYOUTS[layout], out=out.data_ptr(), ldo=_ld(out),
                 out_layout=_OUTS[out_layout], stream=_stream_handle(stream))
        return self.split(out, out_layout)

    def apply_host(self, X, flags=0, out=None, layout="TG", out_layout="TR"):
        """Blocking host form: numpy in, views [level][weighting] of one numpy result out; the field crosses PCIe once
        for all planes (``_lib.HOST_PIN | _lib.HOST_LINES`` as for :meth:`SparsePlan.apply_host`)."""
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64) or X.ndim != 2:
            raise TypeError("X must be a 2-D float32/float64 array")
        T = X.shape[0] if layout == "TG" else X.shape[1]
        shape = (T, self.out_cols) if out_layout == "TR" else (self.out_cols, T)
        out = _host_out(out, shape, X.dtype)
        with _on_device(self.device):
            _lib.run("wagg_apply (many, host)", plan_kind=_lib.PLAN_SEGMENT, plan=self._h, elem=_elem(X.dtype), source=_lib.SRC_HOST,
                     x=X.ctypes.data, T=T, ldx=X.shape[1], layout=_LAYOUTS[layout], out=out.ctypes.data, ldo=max(1, shape[1]),
                     out_layout=_OUTS[out_layout], flags=int(flags))
        return self.split(out, out_layout)


def _exact_flag(exact):
    return _lib.APPLY_EXACT_F32 if exact else 0


class DensePlan:
    """Dense-family plan: W as a (gridcell x region) matrix resident in HBM contracted on the matrix
    cores (full or tile-sparse form; fp32 or fp64 weights), or per-wave entry lists for scattered,
    sparse weights (fp32).  ``info["form"]`` says which (``_lib.FORM_*``), ``dtype`` the element type
    the plan serves ("float32" / "float64")."""

    def __init__(self, handle, G, R, device=None, recipe=None):
        self._h, self.G, self.R = handle, int(G), int(R)
        self.device = _current_device() if device is None else int(device)
        self._recipe = recipe                # synthetic plans: (constructor, args, kwargs) a replica is generated from
        self._lease = threading.Lock()
        den = np.empty(self.R, dtype=np.float64)
        _lib.check(_lib.load().wagg_dense_get_den(self._h, _np_ptr(den, C.c_double)), "wagg_dense_get_den")
        self.den = den
        inf = _lib.DenseInfo()
        _lib.check(_lib.load().wagg_dense_get_info_sized(self._h, C.byref(inf), C.sizeof(inf)), "wagg_dense_get_info_sized")
        self.info = {k: (float if ct is C.c_double else int)(getattr(inf, k)) for k, ct in _lib.DenseInfo._fields_}
        self.dtype = "float64" if self.info["elem_bytes"] == 8 else "float32"

    @staticmethod
    def _is64(dtype):
        return str(dtype).endswith("float64") or dtype is np.float64

    @classmethod
    def synth_blocklocal(cls, G, R, seed, fill=0.952, dtype="float32", device=None):
        """c5's block-local weights, generated on the device in tile-sparse form."""
        require_gpu()
        h = C.c_void_p()
        L = _lib.load()
        fn = L.wagg_dense_create_synth_blocklocal_f64 if cls._is64(dtype) else L.wagg_dense_create_synth_blocklocal
        with _on_device(device):
            dev = _current_device()
            _lib.check(fn(int(G), int(R), int(seed), float(fill), C.byref(h)), "wagg_dense_create_synth_blocklocal")
        return cls(h, G, R, dev, (cls.synth_blocklocal, (G, R, seed), dict(fill=fill, dtype=dtype)))

    @classmethod
    def synth(cls, G, R, seed, fill=1.0, dtype="float32", device=None):
        """W[g, r] = hash_u01(g R + r, seed); with fill < 1 only that fraction of the entries, at
        uniformly random positions (c5's uniform-random structure at fill = 0.01: entry lists)."""
        require_gpu()
        h = C.c_void_p()
        L = _lib.load()
        fn = L.wagg_dense_create_synth_f64 if cls._is64(dtype) else L.wagg_dense_create_synth_sparse
        with _on_device(device):
            dev = _current_device()
            _lib.check(fn(int(G), int(R), int(seed), float(fill), C.byref(h)), "wagg_dense_create_synth")
        return cls(h, G, R, dev, (cls.synth, (G, R, seed), dict(fill=fill, dtype=dtype)))

    @classmethod
    def from_host(cls, W, device=None):
        """From a host (G, R) matrix; a float64 array makes an fp64 plan, anything else fp32."""
        require_gpu()
        W = np.asarray(W)
        h = C.c_void_p()
        with _on_device(device):
            dev = _current_device()
            if W.dtype == np.float64:
                W = np.ascontiguousarray(W)
                _lib.check(_lib.load().wagg_dense_create_host_f64(_np_ptr(W, C.c_double), W.shape[0], W.shape[1], C.byref(h)),
                           "wagg_dense_create_host_f64")
            else:
                W = np.ascontiguousarray(W, dtype=np.float32)
                _lib.check(_lib.load().wagg_dense_create_host(_np_ptr(W, C.c_float), W.shape[0], W.shape[1], C.byref(h)),
                           "wagg_dense_create_host")
        return cls(h, W.shape[0], W.shape[1], dev)

    @classmethod
    def from_segments(cls, cell_idx, region_code, w_eff, G, R, dtype="float32", device=None, form=None):
        """From the coded segment table (COO rows; ``wagg_dense_create_from_segments*``).  ``form``: None / "auto" lets the
        library choose (the caller never needs to know the form, like the reference's single weights type,
        aggregations.py:64-73); "full" / "tiles" / "entries" pin it (measurements, tests).  At most 2**31 - 1 rows."""
        require_gpu()
        ci = np.ascontiguousarray(cell_idx, dtype=np.int32)
        rc = np.ascontiguousarray(region_code, dtype=np.int32)
        we = np.ascontiguousarray(w_eff, dtype=np.float64)
        h = C.c_void_p()
        L = _lib.load()
        fn = L.wagg_dense_create_from_segments_f64 if cls._is64(dtype) else L.wagg_dense_create_from_segments
        with _on_device(device):
            dev = _current_device()
            _lib.check(fn(_np_ptr(ci, C.c_int32), _np_ptr(rc, C.c_int32), _np_ptr(we, C.c_double), len(ci), int(G),
                          int(R), _lib.FORCE_FORM[form], C.byref(h)), "wagg_dense_create_from_segments")
        return cls(h, G, R, dev)

    @classmethod
    def from_csr(cls, rowptr, col, val, G, R, dtype="float32", device=None, form=None, general_sort=False):
        """From a caller's table in CSR form (``wagg_dense_create_from_csr*``; BASELINE configs[4] "sparse CSR weights"):
        ``rowptr`` (G + 1 offsets, rows = grid cells), ``col`` = region codes, ``val`` = fp64 weights -- the coded form of
        the reference's weights table (aggregations.py:64-73).  The arrays are uploaded as they are (no host copy when
        they already have the dtypes int64 / int32 / float64); everything else happens on the device.  ``form`` as for
        :meth:`from_segments`.  A table whose columns ascend inside every row (scipy's ``has_sorted_indices``) is put in
        the plan's order by one stable pass per chunk of 128 cells instead of the general radix sort
        (``info["one_pass_sort"]``); ``general_sort=True`` takes the general sort regardless -- same plan, for tests
        and timings."""
        require_gpu()
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        co = np.ascontiguousarray(col, dtype=np.int32)
        va = np.ascontiguousarray(val, dtype=np.float64)
        if rp.shape != (int(G) + 1,) or co.shape != va.shape or co.ndim != 1 or (len(rp) and int(rp[-1]) != len(co)):
            raise ValueError("rowptr must hold G + 1 offsets ending at len(col) == len(val)")
        h = C.c_void_p()
        L = _lib.load()
        fn = L.wagg_dense_create_from_csr_f64 if cls._is64(dtype) else L.wagg_dense_create_from_csr
        with _on_device(device):
            dev = _current_device()
            _lib.check(fn(_np_ptr(rp, C.c_int64), _np_ptr(co, C.c_int32), _np_ptr(va, C.c_double), int(G), int(R),
                          _lib.FORCE_FORM[form] | (_lib.DENSE_GENERAL_SORT if general_sort else 0), C.byref(h)),
                       "wagg_dense_create_from_csr")
        return cls(h, G, R, dev)

    def replica(self, device):
        """The same weights as a plan of its own on ``device`` (multi-device host streaming; a dense-family plan
        owns its workspaces, so every pipeline needs its own replica -- also two on one device).  Plans built from a
        table or a host matrix are cloned device to device (``wagg_dense_clone``: the packed plan travels, over xGMI
        between two GPUs -- nothing is uploaded or sorted again and no copy of the caller's arrays is kept for it);
        the synthetic generators run again on the target (a 101 GB operand is quicker made than moved)."""
        if self._recipe is not None:
            fn, args, kw = self._recipe
            return fn(*args, device=device, **kw)
        require_gpu()
        h = C.c_void_p()
        _lib.check(_lib.load().wagg_dense_clone(self._h, int(device), C.byref(h)), "wagg_dense_clone")
        return type(self)(h, self.G, self.R, int(device))

    def read_w(self, image=False):
        """The stored tiles as bytes, as they lie on the device (``wagg_dense_read_w``): the packed W, or with ``image`` the f16
        high / low image of a full-form fp32 plan (``info["w_image_bytes"]`` says whether one is held).  For layout tests."""
        fn = _lib.load().wagg_dense_read_w
        buf = np.empty(self.info["w_bytes"], dtype=np.uint8)
        _lib.check(fn(self._h, 1 if image else 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes), "wagg_dense_read_w")
        return buf

    def read_split(self, what, nbytes):
        """The first ``nbytes`` of a split-form workspace as the last apply left it (``wagg_dense_read_w`` with image = 2 / 3):
        ``what`` = "xp", the packed f16 high / low tiles of X, or "xmax", the row maxima as float bits.  The caller has
        waited for the apply.  For layout tests."""
        buf = np.empty(int(nbytes), dtype=np.uint8)
        _lib.check(_lib.load().wagg_dense_read_w(self._h, {"xp": 2, "xmax": 3}[what], buf.ctypes.data_as(C.c_void_p), buf.nbytes),
                   "wagg_dense_read_w")
        return buf

    def close(self):
        for r in getattr(self, "_replicas", {}).values():
            r.close()
        if getattr(self, "_h", None) is not None and self._h.value and _lib is not None and _lib._lib is not None:
            _lib._lib.wagg_dense_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _prep(self, X, out, stream=None):
        import torch
        X = _check_X(X, "TG")
        want = torch.float64 if self.dtype == "float64" else torch.float32
        if X.dtype != want:
            raise TypeError("this dense plan serves %s data, got %s" % (self.dtype, X.dtype))
        if X.shape[1] != self.G:
            raise ValueError("X has %d grid cells, plan expects %d" % (X.shape[1], self.G))
        T = X.shape[0]
        if out is None:
            with _on_stream(stream):
                out = torch.empty((T, self.R), dtype=want, device=X.device)
        elif tuple(out.shape) != (T, self.R) or out.dtype != want or (self.R > 1 and out.stride(1) != 1):
            raise ValueError("out must be a (%d, %d) %s tensor with contiguous rows" % (T, self.R, self.dtype))
        return X, T, out

    def _run(self, what, **fields):
        _lib.run(what, plan_kind=_lib.PLAN_DENSE, elem=_elem(self.dtype), **fields)

    def apply(self, X, out=None, ksplit=0, stream=None, exact=False):
        """``exact=True``: an fp32 full-form plan runs the fp32 MFMA kernel instead of the default split form
        (``WAGG_APPLY_EXACT_F32``; the same for apply_poly / apply_edd / apply_host).  Asynchronous on torch's current stream
        or ``stream``; a new ``out`` then belongs to that stream in torch's allocator (the module's docstring)."""
        X, T, out = self._prep(X, out, stream)
        self._run("wagg_apply (dense)", plan=self._h, source=_lib.SRC_DEVICE, x=X.data_ptr(), T=T, ldx=_ld(X), out=out.data_ptr(),
                  ldo=_ld(out), ksplit=int(ksplit), stream=_stream_handle(stream), flags=_exact_flag(exact))
        return out

    def apply_poly(self, X, offset, power, out=None, ksplit=0, stream=None, exact=False):
        """Aggregate of (X + offset) ** power (``wagg_dense_apply_poly_*``): the transform of
        tas_poly (transformations.py:188) is evaluated while X is packed."""
        X, T, out = self._prep(X, out, stream)
        self._run("wagg_apply (dense, poly)", plan=self._h, source=_lib.SRC_DEVICE, transform=_lib.XF_POLY, offset=float(offset),
                  pow_first=int(power), n_pow=1, x=X.data_ptr(), T=T, ldx=_ld(X), out=out.data_ptr(), ldo=_ld(out), ksplit=int(ksplit),
                  stream=_stream_handle(stream), flags=_exact_flag(exact))
        return out

    def apply_edd(self, tasmin, tasmax, threshold, offset=0.0, out=None, ksplit=0, stream=None, exact=False):
        """Aggregate of snyder_edd(tasmin + offset, tasmax + offset, threshold)
        (``wagg_dense_apply_edd_*``; transformations.py:64-87 evaluated while the fields are packed)."""
        tasmin, T, out = self._prep(tasmin, out, stream)
        tasmax = _check_X(tasmax, "TG")
        if tasmax.shape != tasmin.shape or tasmax.dtype != tasmin.dtype or _ld(tasmax) != _ld(tasmin):
            raise ValueError("tasmin and tasmax must have the same shape, dtype and row stride")
        thr = (C.c_double * 1)(float(threshold))
        self._run("wagg_apply (dense, edd)", plan=self._h, source=_lib.SRC_DEVICE, transform=_lib.XF_EDD, offset=float(offset),
                  thresholds=thr, n_thr=1, x=tasmin.data_ptr(), x2=tasmax.data_ptr(), T=T, ldx=_ld(tasmin), out=out.data_ptr(),
                  ldo=_ld(out), ksplit=int(ksplit), stream=_stream_handle(stream), flags=_exact_flag(exact))
        return out

    def apply_host(self, X, flags=0, replicas=(), out=None, exact=False):
        """Host-resident (time, gridcell) array through the plan in row blocks (``wagg_dense_apply_host_*``):
        numpy in, numpy out; flags and ``replicas`` as for :meth:`SparsePlan.apply_host` (``_lib.HOST_LINES`` means nothing
        to a dense-family plan -- every cell of a row is an operand -- and is dropped)."""
        flags = int(flags) & ~(_lib.HOST_LINES | _lib.HOST_LINES_WHOLE)
        want = np.float64 if self.dtype == "float64" else np.float32
        X = np.ascontiguousarray(X)
        if X.dtype != want or X.ndim != 2 or X.shape[1] != self.G:
            raise TypeError("X must be a (T, %d) %s array" % (self.G, self.dtype))
        out = _host_out(out, (X.shape[0], self.R), want)
        if replicas:
            plans = (self,) + tuple(replicas)
            hs = (C.c_void_p * len(plans))(*[p._h for p in plans])
            devs = (C.c_int32 * len(plans))(*[p.device for p in plans])
            self._run("wagg_apply (dense, host, multi-device)", plan=hs, n_plans=len(plans), devices=devs, source=_lib.SRC_HOST_MULTI,
                      x=X.ctypes.data, T=X.shape[0], ldx=X.shape[1], out=out.ctypes.data, ldo=max(1, self.R), flags=int(flags))
            return out
        with _on_device(self.device):
            self._run("wagg_apply (dense, host)", plan=self._h, source=_lib.SRC_HOST, x=X.ctypes.data, T=X.shape[0], ldx=X.shape[1],
                      out=out.ctypes.data, ldo=max(1, self.R), flags=int(flags) | _exact_flag(exact))
        return out

    def saw_inf(self, stream=None):
        """True when an apply since the last call met +-inf in its (transformed) data in one of the MFMA
        forms (``wagg_dense_saw_inf``; synchronises the stream and clears the note)."""
        saw = C.c_int(0)
        _lib.check(_lib.load().wagg_dense_saw_inf(self._h, _stream_handle(stream), C.byref(saw)), "wagg_dense_saw_inf")
        return bool(saw.value)


class ShardGroup:
    """Time-axis shards of ONE job on several devices driven by this process, device-resident data
    (``wagg_shard_group_*`` / ``wagg_*apply_sharded_*``; SURVEY 8b ``n_devices``, 8e): shard i -- a (rows_i, G) tensor on
    ``devices[i]`` -- goes through ``plans[i]`` (a replica of the table on that device) and its block lands directly in its
    rows of the result on ``devices[root]``; the blocks travel by RCCL (grouped send / receive, every shard to the root on its
    own link) or by peer copies (``transport``: "auto", "rccl", "peer"; a device may be listed twice with "peer").  Blocking.
    The process-per-GPU form of the same job is :mod:`climate_toolbox_amd.timeshard` (``torch.distributed``)."""

    _TRANSPORTS = {"auto": _lib.GATHER_AUTO, "rccl": _lib.GATHER_RCCL, "peer": _lib.GATHER_PEER}

    def __init__(self, devices, transport="auto"):
        require_gpu()
        self.devices = [int(d) for d in devices]
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        self._h = C.c_void_p()
        _lib.check(_lib.load().wagg_shard_group_create(arr, len(self.devices), self._TRANSPORTS[transport], C.byref(self._h)),
                   "wagg_shard_group_create")
        n, tr = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().wagg_shard_group_info(self._h, C.byref(n), C.byref(tr)), "wagg_shard_group_info")
        self.transport = {_lib.GATHER_RCCL: "rccl", _lib.GATHER_PEER: "peer"}[tr.value]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and _lib._lib is not None:
            _lib._lib.wagg_shard_group_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def apply(self, plans, shards, root=0, out=None):
        """``plans[i]`` / ``shards[i]`` per device of the group; returns the (sum rows, R) tensor on ``devices[root]``."""
        import torch
        n = len(self.devices)
        if len(plans) != n or len(shards) != n:
            raise ValueError("the group has %d shards: need as many plans and tensors" % n)
        dense = isinstance(plans[0], DensePlan)
        if any(isinstance(p, DensePlan) != dense for p in plans):
            raise TypeError("all plans of a call are of one family")
        dtype = shards[0].dtype
        rows, lds = [], set()
        for i, x in enumerate(shards):
            if not (x.is_cuda and x.dim() == 2 and x.dtype == dtype and x.device.index == self.devices[i] and x.shape[1] == plans[0].G):
                raise ValueError("shard %d must be a (rows, %d) %s tensor on device %d" % (i, plans[0].G, dtype, self.devices[i]))
            if x.shape[0] and x.shape[1] > 1 and x.stride(1) != 1:
                raise ValueError("shard %d: rows must be contiguous" % i)
            if x.shape[0] > 1:
                lds.add(_ld(x))
            rows.append(int(x.shape[0]))
        if len(lds) > 1:
            raise ValueError("the shards must share one row stride, got %r" % sorted(lds))
        ldx = lds.pop() if lds else plans[0].G
        R = plans[0].R
        total = sum(rows)
        if out is None:
            out = torch.empty((total, R), dtype=dtype, device="cuda:%d" % self.devices[root])
        elif tuple(out.shape) != (total, R) or out.dtype != dtype or out.device.index != self.devices[root] or (R > 1 and out.stride(1) != 1):
            raise ValueError("out must be a (%d, %d) %s tensor on device %d" % (total, R, dtype, self.devices[root]))
        hp = (C.c_void_p * n)(*[p._h for p in plans])
        xp = (C.c_void_p * n)(*[C.c_void_p(x.data_ptr()) for x in shards])
        rw = (C.c_int64 * n)(*rows)
        for d in set(self.devices):                      # the shards' producers ran on torch's streams: the group uses its own
            torch.cuda.synchronize(d)
        _lib.run("wagg_apply (sharded)", plan_kind=_lib.PLAN_DENSE if dense else _lib.PLAN_SEGMENT, plan=hp, n_plans=n, elem=_elem(dtype),
                 source=_lib.SRC_SHARDED, group=self._h, x=xp, rows=rw, ldx=ldx, out=out.data_ptr(), ldo=_ld(out), root=int(root))
        return out


def gather(X, cell_idx_dev, layout="TG", out_layout="TR", stream=None):
    """Materialised pointwise gather (aggregations.py:27) on the device; with ``stream=`` the result belongs to that stream in
    torch's allocator (the module's docstring)."""
    import torch
    X = _check_X(X, layout)
    if not (cell_idx_dev.is_cuda and cell_idx_dev.dtype == torch.int32 and cell_idx_dev.is_contiguous()):
        raise TypeError("cell_idx_dev must be a contiguous int32 CUDA tensor")
    T = X.shape[0] if layout == "TG" else X.shape[1]
    n = cell_idx_dev.numel()
    shape = (T, n) if out_layout == "TR" else (n, T)
    with _on_stream(stream):
        out = torch.empty(shape, dtype=X.dtype, device=X.device)
    L = _lib.load()
    fn = L.wagg_gather_f32 if X.dtype == torch.float32 else L.wagg_gather_f64
    _lib.check(fn(C.c_void_p(X.data_ptr()), T, _ld(X), _LAYOUTS[layout],
                  C.c_void_p(cell_idx_dev.data_ptr()), n, C.c_void_p(out.data_ptr()), max(1, shape[1]),
                  _OUTS[out_layout], _stream_handle(stream)), "wagg_gather")
    return out


# which way the calls of pack_rows went: "device" (the pack kernel on a device tensor), "host" (the gather pipeline from host
# arrays), "host_fallback" (host arrays the gather could not serve: uploaded whole, then the pack kernel)
PACK_STATS = {"device": 0, "host": 0, "host_fallback": 0}


def pack_rows(plan, X, X2=None, stream=None):
    """The rows of a (T, G) field with only the quads the plan's table references: a (T, Gq) CUDA tensor, column ``j`` being cell
    ``plan.compact_cells(X.dtype)[j]`` (``wagg_pack_rows_*``).  With ``X2`` (tasmax beside tasmin; same shape, dtype and row
    stride) a (T, 2 Gq) tensor: field 0 in ``[:, :Gq]``, field 1 in ``[:, Gq:]``.  ``X`` / ``X2``: CUDA tensors (asynchronous on
    torch's current stream, or ``stream`` -- the result then belongs to that stream in torch's allocator, see the module's
    docstring) or NumPy arrays -- then host threads pack the quads and only they cross PCIe
    (``wagg_pack_rows_host_*``; blocking) where the library takes that way (a field of >= 64 MiB whose packed row is <= 80 % of
    the row, enough CPUs), and the field is uploaded whole and packed on the device where it does not.  ``PACK_STATS`` counts
    the ways taken.  WaggError for a plan without a compact row."""
    torch = require_gpu()
    if not isinstance(plan, SparsePlan):
        raise TypeError("pack_rows takes a SparsePlan")
    on_host = not isinstance(X, torch.Tensor)
    if on_host:
        X = np.ascontiguousarray(X)
        X2 = None if X2 is None else np.ascontiguousarray(X2)
        if X.dtype not in (np.float32, np.float64) or X.ndim != 2:
            raise TypeError("X must be a 2-D float32/float64 array or CUDA tensor")
    else:
        X = _check_X(X, "TG")
        X2 = None if X2 is None else _check_X(X2, "TG")
    if X2 is not None and (isinstance(X2, torch.Tensor) == on_host or tuple(X2.shape) != tuple(X.shape) or X2.dtype != X.dtype):
        raise ValueError("X and X2 must have the same residency, shape and dtype")
    if X.shape[1] != plan.G:
        raise ValueError("X has %d grid cells, plan expects %d" % (X.shape[1], plan.G))
    cells = plan.compact_cells(X.dtype)
    if cells is None:
        raise WaggError("this plan has no compact row for %s data" % (X.dtype,))
    T, nf, f32 = int(X.shape[0]), 1 if X2 is None else 2, _elem(X.dtype) == _lib.T_F32
    L = _lib.load()
    with _on_device(plan.device):
        if on_host:
            out = torch.empty((T, nf * len(cells)), dtype=torch.float32 if f32 else torch.float64, device="cuda")
            torch.cuda.current_stream().synchronize()      # (the caching allocator may hand out memory the stream still writes)
            fn = L.wagg_pack_rows_host_f32 if f32 else L.wagg_pack_rows_host_f64
            rc = fn(plan._h, C.c_void_p(X.ctypes.data), None if X2 is None else C.c_void_p(X2.ctypes.data), T, X.shape[1],
                    C.c_void_p(out.data_ptr()), max(1, out.shape[1]), 0)
            if rc != _lib.EUNSUPPORTED:
                _lib.check(rc, "wagg_pack_rows_host")
                PACK_STATS["host"] += 1
                return out
            PACK_STATS["host_fallback"] += 1
            X, X2 = upload(X), None if X2 is None else upload(X2)
        else:
            if X2 is not None and _ld(X2) != _ld(X):
                raise ValueError("X and X2 must share one row stride")
            with _on_stream(stream):
                out = torch.empty((T, nf * len(cells)), dtype=X.dtype, device=X.device)
            PACK_STATS["device"] += 1
        fn = L.wagg_pack_rows_f32 if f32 else L.wagg_pack_rows_f64
        _lib.check(fn(plan._h, C.c_void_p(X.data_ptr()), None if X2 is None else C.c_void_p(X2.data_ptr()), T, _ld(X),
                      C.c_void_p(out.data_ptr()), max(1, out.shape[1]), _stream_handle(stream)), "wagg_pack_rows")
        if stream is not None:
            for t in (X, X2):
                if t is not None:
                    t.record_stream(stream)
    return out


def _flat_dev(t, stream=None):
    """``t`` itself when it is contiguous, else its contiguous copy made on ``stream`` (:func:`relayout`)"""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.float32, torch.float64)):
        raise TypeError("expected a float32/float64 CUDA tensor")
    return t if t.is_contiguous() else relayout(t, stream=stream)


def transform_poly(X, offset, power, stream=None):
    """(X + offset) ** power elementwise on the device (``wagg_transform_poly_*``; the arithmetic of
    tas_poly, transformations.py:188, as the fused kernels evaluate it)."""
    import torch
    X = _flat_dev(X, stream)
    with _on_stream(stream):
        out = torch.empty_like(X)
    L = _lib.load()
    fn = L.wagg_transform_poly_f32 if X.dtype == torch.float32 else L.wagg_transform_poly_f64
    _lib.check(fn(C.c_void_p(X.data_ptr()), X.numel(), float(offset), int(power), C.c_void_p(out.data_ptr()),
                  _stream_handle(stream)), "wagg_transform_poly")
    return out


def transform_edd(tasmin, tasmax, offset, terms, stream=None):
    """sum_k coef_k * snyder_edd(tasmin + offset, tasmax + offset, threshold_k) elementwise on the
    device (``wagg_transform_edd_*``; transformations.py:64-87, :138-140)."""
    import torch
    lo, hi = _flat_dev(tasmin, stream), _flat_dev(tasmax, stream)
    if lo.shape != hi.shape or lo.dtype != hi.dtype:
        raise ValueError("tasmin and tasmax must have the same shape and dtype")
    coefs = np.ascontiguousarray([c for c, _ in terms], dtype=np.float64)
    thr = np.ascontiguousarray([e for _, e in terms], dtype=np.float64)
    with _on_stream(stream):
        out = torch.empty_like(lo)
    L = _lib.load()
    fn = L.wagg_transform_edd_f32 if lo.dtype == torch.float32 else L.wagg_transform_edd_f64
    _lib.check(fn(C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), lo.numel(), float(offset),
                  _np_ptr(coefs, C.c_double), _np_ptr(thr, C.c_double), len(coefs), C.c_void_p(out.data_ptr()),
                  _stream_handle(stream)), "wagg_transform_edd")
    return out


def combine_planes(stack, coefs, stream=None):
    """sum_k coefs[k] * stack[k] on the device (``wagg_combine_planes_*``): how the aggregated degree days of several
    thresholds become snyder_gdd (transformations.py:138-140).  ``stack``: contiguous (K, ...) CUDA tensor, K <= 8."""
    import torch
    if not (isinstance(stack, torch.Tensor) and stack.is_cuda and stack.is_contiguous() and stack.dtype in (torch.float32, torch.float64)):
        raise TypeError("stack must be a contiguous float32/float64 CUDA tensor")
    cf = np.ascontiguousarray(coefs, dtype=np.float64)
    if len(cf) != stack.shape[0]:
        raise ValueError("one coefficient per plane")
    with _on_stream(stream):
        out = torch.empty(stack.shape[1:], dtype=stack.dtype, device=stack.device)
    L = _lib.load()
    fn = L.wagg_combine_planes_f32 if stack.dtype == torch.float32 else L.wagg_combine_planes_f64
    n = out.numel()
    _lib.check(fn(C.c_void_p(stack.data_ptr()), len(cf), n, _np_ptr(cf, C.c_double), n, C.c_void_p(out.data_ptr()),
                  _stream_handle(stream)), "wagg_combine_planes")
    return out


def period_lists(row_begin, rows, T, device=None):
    """Host row lists (CSR: ``row_begin`` of P + 1 offsets into ``rows``) checked against ``T`` rows and uploaded as the two
    int32 CUDA tensors :func:`period_reduce` takes; ValueError for offsets that do not ascend or a row outside [0, T)."""
    import torch
    rb = np.ascontiguousarray(row_begin, dtype=np.int64)
    rw = np.ascontiguousarray(rows, dtype=np.int64)
    if rb.ndim != 1 or rw.ndim != 1 or len(rb) < 1 or rb[0] < 0 or rb[-1] > len(rw) or (np.diff(rb) < 0).any():
        raise ValueError("row_begin must hold P + 1 ascending offsets into rows")
    if len(rw) and (rw.min() < 0 or rw.max() >= int(T)):
        raise ValueError("a period lists a row outside [0, %d)" % int(T))
    dev = "cuda" if device is None else device
    return torch.from_numpy(rb.astype(np.int32)).to(dev), torch.from_numpy(rw.astype(np.int32)).to(dev)


def _season_vector(a, length, what, device):
    """``a`` (host integers or an int32 CUDA tensor) as the contiguous int32 CUDA tensor of ``length`` entries the season calls take"""
    import torch
    if not isinstance(a, torch.Tensor):
        h = np.ascontiguousarray(a)
        if h.ndim != 1 or h.dtype.kind not in "iu":
            raise TypeError("%s must be a 1-D integer array or an int32 CUDA tensor" % what)
        if len(h) and (h.min() < np.iinfo(np.int32).min or h.max() > np.iinfo(np.int32).max):
            raise ValueError("%s must fit int32" % what)
        a = torch.from_numpy(h.astype(np.int32)).to(device)
    if not (a.is_cuda and a.dtype == torch.int32 and a.dim() == 1 and a.is_contiguous()):
        raise TypeError("%s must be a contiguous int32 CUDA tensor (or host integers)" % what)
    if int(a.numel()) != int(length):
        raise ValueError("%s must hold %d entries, got %d" % (what, int(length), int(a.numel())))
    return a


class _RowlistCall:
    """What the nine row-list calls -- :func:`period_reduce`, :func:`season_reduce` and, through :func:`_grouped_reduce`,
    :func:`edd_ladder_reduce`, :func:`exposure_reduce`, :func:`bin_days_reduce`, :func:`hinge_reduce`, :func:`spell_reduce`, :func:`rolling_reduce` and :func:`quantile_select` -- do alike around
    their library call, in the order they do it: the row lists (and, with ``season = (doy, windows)``, those two vectors) as int32 CUDA tensors and ``P``;
    then ``out``, ``status`` and the workspace; at the end what must outlive the kernels on the caller's stream."""

    def __init__(self, X, row_begin, rows, checked, season=None):
        import torch
        self.X, self.T, self.n = X, int(X.shape[0]), int(X.shape[1])
        if not (isinstance(row_begin, torch.Tensor) and isinstance(rows, torch.Tensor)):
            row_begin, rows = period_lists(row_begin, rows, self.T, device=X.device)
            checked = True
        for a in (row_begin, rows):
            if not (a.is_cuda and a.dtype == torch.int32 and a.dim() == 1 and a.is_contiguous()):
                raise TypeError("row_begin and rows must be contiguous int32 CUDA tensors (or host integers)")
        doy = windows = None
        if season is not None:
            doy = _season_vector(season[0], self.T, "doy", X.device)
            windows = _season_vector(season[1], self.n, "windows", X.device)
        self.row_begin, self.rows, self.doy, self.windows, self.work = row_begin, rows, doy, windows, None
        self.n_rows, self.P = int(rows.numel()), int(row_begin.numel()) - 1
        self.flags = _lib.PERIOD_ROWS_CHECKED if checked else 0
        if self.P < 0:
            raise ValueError("row_begin must hold P + 1 offsets")

    def alloc(self, work_bytes, planes, out, status, workspace=True, stream=None):
        """``(out, status, work pointer, work bytes)``; ``work_bytes``: the library's ``*_work_bytes`` for this call
        (``workspace=False``: the library gets no scratch and sums every period's list in one part).  ``stream``: the stream the
        library call will run on -- the zero-fill of a new status word is queued there, ahead of the kernel that sets its bits"""
        import torch
        X, shape = self.X, (planes, self.P, self.n)
        if out is not None and (tuple(out.shape) != shape or out.dtype != X.dtype or not out.is_contiguous()):
            raise ValueError("out must be a contiguous %s %s tensor" % (shape, X.dtype))
        wb = int(work_bytes(self.n, self.P, self.n_rows, planes)) if workspace else 0
        with _on_stream(stream):
            if out is None:
                out = torch.empty(shape, dtype=X.dtype, device=X.device)
            if status is None:
                status = torch.zeros(1, dtype=torch.int32, device=X.device)
            self.work = torch.empty(wb // 8, dtype=torch.float64, device=X.device) if wb else None
        return out, status, None if self.work is None else C.c_void_p(self.work.data_ptr()), wb

    def done(self, stream):
        if stream is not None:                       # scratch and lists go back to torch's allocator on return: keep them alive
            for t in (self.work, self.row_begin, self.rows, self.doy, self.windows):     # until the kernels on the caller's
                if t is not None:                                                        # stream are through with them
                    t.record_stream(stream)


def _rowlist_transform(X, X2, poly, edd):
    """``poly=`` / ``edd=`` of the four-plane calls as ``(transform, offset, pow_first, n_pow, thresholds, planes, X2)``"""
    transform, offset, pow_first, n_pow, thr, planes = _lib.XF_NONE, 0.0, 1, 1, None, 1
    if poly is not None and edd is not None:
        raise ValueError("one transform per call")
    if poly is not None:
        transform, (offset, pow_first, n_pow) = _lib.XF_POLY, poly
        planes = int(n_pow)
    elif edd is not None:
        transform, offset = _lib.XF_EDD, edd[0]
        thr = np.ascontiguousarray(np.atleast_1d(edd[1]), dtype=np.float64)
        planes = len(thr)
        X2 = _check_X(X2, "TG")
        if X2.shape != X.shape or X2.dtype != X.dtype or _ld(X2) != _ld(X):
            raise ValueError("tasmin and tasmax must have the same shape, dtype and row stride")
    if not 1 <= planes <= 4:
        raise ValueError("1..4 planes per call, got %d" % planes)
    return transform, float(offset), int(pow_first), int(n_pow), thr, planes, X2


def period_reduce(X, row_begin, rows, X2=None, poly=None, edd=None, keep_nan=False, checked=False, out=None, status=None, stream=None,
                  workspace=True):
    """Period totals of the rows of a (T, n) CUDA tensor (``wagg_period_reduce_*``): ``out[k, p, j] = sum_t f_k(X[t, j])`` over
    the rows ``t`` of period ``p`` in list order, fp64 accumulation.  ``row_begin`` / ``rows``: the CSR row lists -- host
    integers (checked here, uploaded) or the int32 CUDA tensors of :func:`period_lists` (``checked=True``: the call is then
    asynchronous; otherwise the library checks them on the device first, which blocks).  ``poly=(offset, pow_first, n_pow)``:
    planes ``(x + offset) ** q``; ``edd=(offset, thresholds)`` with ``X2`` = tasmax: Snyder degree days per threshold; neither:
    one plane of plain sums.  ``keep_nan``: NaN propagates (sums of aggregated results) instead of counting 0 (S6).
    ``workspace=False``: no scratch for the library, so a period's list is never cut into parts -- the split then does not depend
    on ``n``, and a column's sum has the same bits whatever matrix it sits in (here and in the two calls below).
    Returns ``(out, status)``: the (planes, P, n) tensor and the one-word int32 CUDA tensor ``status`` (zeroed here unless
    handed in), bit 0 of which the kernel sets when a transformed value was +-inf -- reading it waits for the kernel.  With
    ``stream=`` everything runs there, the zero-fill of ``status`` included, and the tensors allocated here belong to that
    stream in torch's allocator (the module's docstring; the same for every row-list call below)."""
    import torch
    X = _check_X(X, "TG")
    c = _RowlistCall(X, row_begin, rows, checked)
    transform, offset, pow_first, n_pow, thr, planes, X2 = _rowlist_transform(X, X2, poly, edd)
    L = _lib.load()
    out, status, work, wb = c.alloc(L.wagg_period_reduce_work_bytes, planes, out, status, workspace, stream)
    fn = L.wagg_period_reduce_f32 if X.dtype == torch.float32 else L.wagg_period_reduce_f64
    _lib.check(fn(C.c_void_p(X.data_ptr()), C.c_void_p(X2.data_ptr()) if edd is not None else None, c.T, c.n, _ld(X),
                  C.c_void_p(c.row_begin.data_ptr()), C.c_void_p(c.rows.data_ptr()), c.P, c.n_rows, transform, offset, pow_first, n_pow,
                  None if thr is None else _np_ptr(thr, C.c_double), 0 if thr is None else len(thr),
                  (_lib.PERIOD_KEEP_NAN if keep_nan else 0) | c.flags, C.c_void_p(out.data_ptr()), max(1, c.n), max(1, c.P * c.n),
                  C.c_void_p(status.data_ptr()), work, wb, _stream_handle(stream)), "wagg_period_reduce")
    c.done(stream)
    return out, status


def season_reduce(X, row_begin, rows, doy, windows, X2=None, poly=None, edd=None, checked=False, out=None, status=None, stream=None,
                  workspace=True):
    """Growing-season totals of the rows of a (T, n) CUDA tensor (``wagg_season_reduce_*``): :func:`period_reduce` with one more
    predicate -- ``out[k, p, j]`` sums ``f_k(X[t, j])`` over the rows ``t`` of period ``p`` on which cell ``j`` is in season.
    ``doy``: the day of year of each of the T rows; ``windows``: one packed window per cell (``_lib.SEASON_*``: bits 0-9 first
    day, 10-19 last day, bit 20 invert, bit 21 null; :func:`climate_toolbox_amd.seasons.season_windows` builds them) -- host
    integers or int32 CUDA tensors.  Everything else as for :func:`period_reduce`, without ``keep_nan``: NaN in season counts 0
    (S6), a value out of season is never looked at.  Returns ``(out, status)``; bit 0 of ``status``: an in-season transformed
    value was +-inf."""
    import torch
    X = _check_X(X, "TG")
    c = _RowlistCall(X, row_begin, rows, checked, (doy, windows))
    transform, offset, pow_first, n_pow, thr, planes, X2 = _rowlist_transform(X, X2, poly, edd)
    L = _lib.load()
    out, status, work, wb = c.alloc(L.wagg_season_reduce_work_bytes, planes, out, status, workspace, stream)
    fn = L.wagg_season_reduce_f32 if X.dtype == torch.float32 else L.wagg_season_reduce_f64
    _lib.check(fn(C.c_void_p(X.data_ptr()), C.c_void_p(X2.data_ptr()) if edd is not None else None, c.T, c.n, _ld(X),
                  C.c_void_p(c.row_begin.data_ptr()), C.c_void_p(c.rows.data_ptr()), c.P, c.n_rows, C.c_void_p(c.doy.data_ptr()),
                  C.c_void_p(c.windows.data_ptr()), transform, offset, pow_first, n_pow,
                  None if thr is None else _np_ptr(thr, C.c_double), 0 if thr is None else len(thr), c.flags,
                  C.c_void_p(out.data_ptr()), max(1, c.n), max(1, c.P * c.n), C.c_void_p(status.data_ptr()), work, wb,
                  _stream_handle(stream)), "wagg_season_reduce")
    c.done(stream)
    return out, status


def _grouped_reduce(name, fields, row_begin, rows, doy, windows, checked, offset, middle, planes, work_bytes, out, status, workspace,
                    stream):
    """What :func:`edd_ladder_reduce`, :func:`exposure_reduce`, :func:`bin_days_reduce`, :func:`hinge_reduce`,
    :func:`spell_reduce`, :func:`rolling_reduce` and :func:`quantile_select` do alike behind their own validation: the doy / windows pairing, the :class:`_RowlistCall`, ``out`` / ``status`` / workspace, and the library call ``name`` + ``_f32``
    or ``_f64`` by the dtype of ``fields`` (one checked (T, n) tensor, or tasmin and tasmax) -- the fields and the arguments
    every grouped entry point begins with (sizes, lists, season, ``offset``), the family's ``middle`` ones, and the ones every
    one ends with (flags, ``out`` and its strides, status, workspace, stream).  ``work_bytes(L, n, P, n_rows, planes)``: the
    family's ``*_work_bytes``.  Returns ``(out, status)``."""
    import torch
    if (doy is None) != (windows is None):
        raise ValueError("doy and windows go together: both given, or both None (no season)")
    X = fields[0]
    c = _RowlistCall(X, row_begin, rows, checked, None if doy is None else (doy, windows))
    L = _lib.load()
    out, status, work, wb = c.alloc(lambda *a: work_bytes(L, *a), planes, out, status, workspace, stream)
    fn = getattr(L, name + ("_f32" if X.dtype == torch.float32 else "_f64"))
    _lib.check(fn(*[C.c_void_p(f.data_ptr()) for f in fields], c.T, c.n, _ld(X), C.c_void_p(c.row_begin.data_ptr()),
                  C.c_void_p(c.rows.data_ptr()), c.P, c.n_rows, None if doy is None else C.c_void_p(c.doy.data_ptr()),
                  None if doy is None else C.c_void_p(c.windows.data_ptr()), float(offset), *middle, c.flags, C.c_void_p(out.data_ptr()),
                  max(1, c.n), max(1, c.P * c.n), C.c_void_p(status.data_ptr()), work, wb, _stream_handle(stream)), name)
    c.done(stream)
    return out, status


def edd_ladder_reduce(tasmin, tasmax, row_begin, rows, offset, thresholds, doy=None, windows=None, checked=False, out=None, status=None,
                      stream=None, workspace=True):
    """Snyder degree days at every threshold of a ladder, summed per period, in ONE launch (``wagg_edd_ladder_reduce_*``):
    ``out[k, p, j]`` sums ``snyder_edd(tasmin[t, j] + offset, tasmax[t, j] + offset, thresholds[k])`` over the rows ``t`` of
    period ``p`` on which cell ``j`` is in season -- :func:`season_reduce` with ``edd=`` without its cap of four thresholds
    (1 .. ``_lib.EDD_LADDER_MAX``; the kernel takes them ``EDD_LADDER_GROUP`` at a time).  ``tasmin`` / ``tasmax``: (T, n) CUDA
    tensors of one dtype and row stride; ``row_begin`` / ``rows`` / ``doy`` / ``windows`` / ``checked`` as for
    :func:`season_reduce`; ``doy`` and ``windows`` both None: no season, every listed row counts (:func:`period_reduce`).  Plane
    ``k`` is bit for bit the plane those two give for ``thresholds[k]``.  Returns ``(out, status)``: the (n_thr, P, n) tensor and
    the status word (bit 0: an in-season value was +-inf)."""
    X = _check_X(tasmin, "TG")
    X2 = _check_X(tasmax, "TG")
    if X2.shape != X.shape or X2.dtype != X.dtype or _ld(X2) != _ld(X) or X2.device != X.device:
        raise ValueError("tasmin and tasmax must have the same shape, dtype, row stride and device")
    thr = np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
    if thr.ndim != 1 or not 1 <= len(thr) <= _lib.EDD_LADDER_MAX:
        raise ValueError("1..%d thresholds per call, got %s" % (_lib.EDD_LADDER_MAX, thr.shape))
    return _grouped_reduce("wagg_edd_ladder_reduce", (X, X2), row_begin, rows, doy, windows, checked, offset,
                           (_np_ptr(thr, C.c_double), len(thr)), len(thr),
                           lambda L, *a: L.wagg_edd_ladder_work_bytes(*a), out, status, workspace, stream)


def exposure_reduce(tasmin, tasmax, row_begin, rows, offset, edges, doy=None, windows=None, checked=False, out=None, status=None,
                    stream=None, workspace=True):
    """The time a day's sinusoidal temperature curve spends in each bin, summed per period, in ONE launch
    (``wagg_exposure_reduce_*``): ``out[k, p, j]`` sums ``A(edges[k]) - A(edges[k + 1])`` over the rows ``t`` of period ``p`` on
    which cell ``j`` is in season, ``A(e)`` being the fraction of the day the single sine through ``tasmin[t, j] + offset`` and
    ``tasmax[t, j] + offset`` (:func:`edd_ladder_reduce`'s model; ``A = -d EDD / de``) lies above ``e``: 0 for a NaN in either
    field, exactly 1 where tasmin is not below ``e``, exactly 0 where tasmax is not above it, ``acos(z) / pi`` between.
    ``tasmin`` / ``tasmax``: (T, n) CUDA tensors of one dtype and row stride; ``edges``: 2 .. ``_lib.EXPOSURE_EDGES_MAX``
    strictly ascending numbers, ``-inf`` allowed first and ``+inf`` last (the kernel takes the bins ``_lib.EXPOSURE_GROUP`` at a
    time), converted to the element type; everything else as for :func:`edd_ladder_reduce`.  Returns ``(bins, status)``: the
    (n_bins, P, n) tensor in days and the status word (bit 0: an in-season value of either field was +-inf)."""
    X = _check_X(tasmin, "TG")
    X2 = _check_X(tasmax, "TG")
    if X2.shape != X.shape or X2.dtype != X.dtype or _ld(X2) != _ld(X) or X2.device != X.device:
        raise ValueError("tasmin and tasmax must have the same shape, dtype, row stride and device")
    e = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
    if e.ndim != 1 or not 2 <= len(e) <= _lib.EXPOSURE_EDGES_MAX:
        raise ValueError("2..%d bin edges per call, got %s" % (_lib.EXPOSURE_EDGES_MAX, e.shape))
    if np.isnan(e).any() or not (e[1:] > e[:-1]).all():
        raise ValueError("bin edges must ascend strictly and hold no NaN, got %r" % (e.tolist(),))
    return _grouped_reduce("wagg_exposure_reduce", (X, X2), row_begin, rows, doy, windows, checked, offset,
                           (_np_ptr(e, C.c_double), len(e)), len(e) - 1,
                           lambda L, n, P, n_rows, planes: L.wagg_exposure_work_bytes(n, P, n_rows, planes + 1),      # (it takes n_edges)
                           out, status, workspace, stream)


def bin_thresholds(edges, offset, dtype):
    """The thresholds ``wagg_bin_days_reduce_*`` compares the raw field against, restated: ``ceilT(edges[k] - offset)``, the
    difference taken in fp64 and ``ceilT(c)`` the smallest value of ``dtype`` (float32 or float64) that is not below ``c`` --
    ``float32(c)``, stepped up once where that lies below ``c``; infinities pass through.  For every ``x`` of ``dtype``,
    ``x >= ceilT(c)`` holds exactly when ``float64(x) >= c``."""
    c = np.asarray(edges, dtype=np.float64) - np.float64(offset)
    if np.dtype(dtype) == np.float64:
        return c
    if np.dtype(dtype) != np.float32:
        raise TypeError("dtype must be float32 or float64")
    with np.errstate(over="ignore"):
        f = c.astype(np.float32)                       # (to nearest; beyond the largest float: +-inf)
    below = f.astype(np.float64) < c
    return np.where(below, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def bin_days_reduce(X, row_begin, rows, offset, edges, doy=None, windows=None, checked=False, out=None, status=None, workspace=None,
                    stream=None):
    """The days a cell spends in each temperature bin, per period, in ONE launch (``wagg_bin_days_reduce_*``): ``out[k, p, j]``
    counts the rows ``t`` of period ``p`` on which cell ``j`` is in season and ``edges[k] <= X[t, j] + offset < edges[k + 1]``.
    ``X``: a (T, n) CUDA tensor; ``edges``: 2 .. ``_lib.BIN_EDGES_MAX`` strictly ascending numbers, ``-inf`` allowed first and
    ``+inf`` last (the kernel takes the bins ``_lib.BIN_GROUP`` at a time); ``row_begin`` / ``rows`` / ``doy`` / ``windows`` /
    ``checked`` as for :func:`edd_ladder_reduce` (``doy`` and ``windows`` both None: no season).  The comparison is that of
    :func:`bin_thresholds`: the raw value against ``ceilT(edges[k] - offset)``, so an fp32 field is binned as its exact values
    would be in fp64.  NaN is in no bin, ``-inf`` only in a first bin open below, ``+inf`` in none.  ``workspace`` (None = True:
    the library gets the scratch its ``*_work_bytes`` reports; False: none) never changes a count.  Returns ``(counts,
    status)``: the (n_bins, P, n) tensor of ``X``'s dtype (exact in fp32 up to 2^24 days) and the status word (bit 0: an
    in-season value was +-inf)."""
    X = _check_X(X, "TG")
    e = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
    if e.ndim != 1 or not 2 <= len(e) <= _lib.BIN_EDGES_MAX:
        raise ValueError("2..%d bin edges per call, got %s" % (_lib.BIN_EDGES_MAX, e.shape))
    if np.isnan(e).any() or not (e[1:] > e[:-1]).all():
        raise ValueError("bin edges must ascend strictly and hold no NaN, got %r" % (e.tolist(),))
    return _grouped_reduce("wagg_bin_days_reduce", (X,), row_begin, rows, doy, windows, checked, offset,
                           (_np_ptr(e, C.c_double), len(e)), len(e) - 1,
                           lambda L, n, P, n_rows, planes: L.wagg_bin_days_work_bytes(n, P, n_rows, planes + 1),      # (it takes n_edges)
                           out, status, True if workspace is None else workspace, stream)


_SPELL_STATS = {"days": _lib.SPELL_DAYS, "events": _lib.SPELL_EVENTS, "longest": _lib.SPELL_LONGEST}


def _check_side(side):
    if side not in ("above", "below"):
        raise ValueError("side must be 'above' or 'below', got %r" % (side,))


def _spell_codes(stats, stat, side, min_length):
    """``stat`` (a key of ``stats``, the table of a spell call's statistics), ``side`` and ``min_length`` of a spell call, checked
    in that order -- else ValueError; ``"longest"`` takes no ``min_length`` but 1.  Returns what the call's ``middle`` ends with:
    ``(min_length, stat code, below)``."""
    if stat not in stats:
        names = [repr(s) for s in stats]
        raise ValueError("stat must be %s or %s, got %r" % (", ".join(names[:-1]), names[-1], stat))
    _check_side(side)
    if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)) or not 1 <= min_length <= _lib.SPELL_MIN_LENGTH_MAX:
        raise ValueError("min_length must be an integer in 1..%d, got %r" % (_lib.SPELL_MIN_LENGTH_MAX, min_length))
    if stat == "longest" and min_length != 1:
        raise ValueError("stat='longest' does not use min_length: it must be 1, got %r" % (min_length,))
    return int(min_length), stats[stat], 0 if side == "above" else 1


def spell_reduce(X, row_begin, rows, offset, thresholds, min_length=1, stat="days", side="above", doy=None, windows=None, checked=False,
                 out=None, status=None, stream=None, span="period"):
    """Runs of consecutive days past every threshold of a list, per period, in ONE launch (``wagg_spell_reduce_*``).  Entry ``i``
    of period ``p``'s list is hot for cell ``j`` and threshold ``k`` when its row ``t`` lies in the field, the cell is in season
    on ``doy[t]`` and ``X[t, j] + offset >= thresholds[k]`` (``side="above"``) or ``< thresholds[k]`` (``"below"``); a run is a
    maximal stretch of hot entries whose row numbers ascend by one.  A gap in the row numbers, an out-of-season day, a NaN and
    the end of the period's list end a run: runs are truncated at period boundaries.  ``out[k, p, j]`` is, by ``stat``:
    ``"days"`` the hot entries in runs of at least ``min_length``, ``"events"`` the number of such runs, ``"longest"`` the
    length of the longest run (``min_length`` must then be 1).  ``X``: a (T, n) CUDA tensor; ``thresholds``: 1 ..
    ``_lib.SPELL_MAX`` finite numbers in any order, duplicates allowed (the kernel takes them ``_lib.SPELL_GROUP`` at a time);
    ``min_length``: 1 .. ``_lib.SPELL_MIN_LENGTH_MAX``; ``row_begin`` / ``rows`` / ``doy`` / ``windows`` / ``checked`` as for
    :func:`bin_days_reduce`.  The comparison is that of :func:`bin_thresholds`: the raw value against ``ceilT(thresholds[k] -
    offset)``, so an fp32 field is classified as its exact values would be in fp64; NaN is never hot.  There is no workspace:
    a run does not add across the parts of a list, so a period's list is never split.  Returns ``(counts, status)``: the
    (n_thr, P, n) tensor of ``X``'s dtype (exact in fp32 up to 2^24) and the status word (bit 0: an in-season value was
    +-inf, hot or not).

    ``span="record"`` (``wagg_spell_span_*``; anything but ``"period"`` or ``"record"`` is ValueError): RUNS ARE NOT
    TRUNCATED.  The CHAIN is the concatenation of the periods' lists in period order.  Entry ``i`` is hot as above; it JOINS entry
    ``i - 1`` of the chain when ``rows[i] == rows[i - 1] + 1``, whether or not a period boundary or several empty periods lie
    between them (empty lists are transparent); a RUN is a maximal stretch of hot, joined entries of the chain; the RUNNING LENGTH
    ``r_i`` is the entry's position within its run, from 1, or 0 when cold, and is carried over boundaries; ``l`` is the run's
    WHOLE LENGTH.  With ``L = min_length``, ``out[k, p, j]`` is, for ``"days"``: the hot entries of ``p``'s list whose run has
    ``l >= L`` (every day counts in its own period; whether it counts is decided by the whole run); ``"events"``: the entries of
    ``p``'s list with ``r_i == L`` (a run counts once, in the period in which it reaches ``min_length``); ``"longest"``: the
    greatest ``r_i`` over the entries of ``p``'s list, 0 for an empty list (a spell counts in a period for as long as it has
    lasted by then, reaching back to its start wherever that lies).  Where no run crosses a boundary the result is
    ``span="period"``'s bit for bit; summed (``"longest"``: maximised) over the periods it is the ``span="period"`` result of
    the chain taken as one list.  One launch whose blocks each walk the whole record: the grid has no period dimension."""
    if span not in ("period", "record"):
        raise ValueError("span must be 'period' or 'record', got %r" % (span,))
    X = _check_X(X, "TG")
    thr = np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
    if thr.ndim != 1 or not 1 <= len(thr) <= _lib.SPELL_MAX:
        raise ValueError("1..%d thresholds per call, got %s" % (_lib.SPELL_MAX, thr.shape))
    if not np.isfinite(thr).all():
        raise ValueError("thresholds must be finite, got %r" % (thr.tolist(),))
    codes = _spell_codes(_SPELL_STATS, stat, side, min_length)
    return _grouped_reduce("wagg_spell_reduce" if span == "period" else "wagg_spell_span", (X,), row_begin, rows, doy, windows,
                           checked, offset, (_np_ptr(thr, C.c_double), len(thr)) + codes,
                           len(thr), lambda L, *a: L.wagg_spell_work_bytes(*a), out, status, False, stream)


_ROLL_STATS = {"max": _lib.ROLL_MAX, "min": _lib.ROLL_MIN}
_ROLL_OF = {"mean": _lib.ROLL_MEAN, "sum": _lib.ROLL_SUM}


def rolling_reduce(X, row_begin, rows, offset, lengths, stat="max", of="mean", doy=None, windows=None, checked=False, out=None,
                   status=None, stream=None):
    """The greatest (``stat="max"``) or least (``"min"``) running mean (``of="mean"``) or sum (``"sum"``) over ``W`` consecutive
    days, per period, for every ``W`` of ``lengths`` in ONE launch (``wagg_rolling_reduce_*``).  The window lengths are called
    ``lengths`` here because ``windows`` is, as in every other row-list call, the vector of packed SEASON windows (with ``doy``).
    Entry ``i`` of period ``p``'s list is valid for cell ``j`` when its row ``t`` lies in the field, the cell is in season on
    ``doy[t]`` and ``X[t, j]`` is not NaN; a window of ``W`` days ends at entry ``i`` when the entries ``i - W + 1 .. i`` all lie
    in this period's list, their row numbers ascend by one and all are valid.  A gap in the row numbers, an out-of-season day, a
    NaN and the start of the list invalidate every window that would hold them: windows never reach across a period boundary.
    The sum of a window is formed in fp64 from the raw elements, newest to oldest; ``out[k, p, j]`` is the extreme ``m`` of the
    sums of the windows of ``lengths[k]`` days as ``m / W + offset`` (mean) or ``m + W * offset`` (sum), rounded once to ``X``'s
    dtype -- and NaN when the period holds no valid window of that length for the cell.  ``X``: a (T, n) CUDA tensor;
    ``lengths``: 1 .. ``_lib.ROLL_MAX_WINDOWS`` integers in 1 .. ``_lib.ROLL_WINDOW_MAX`` in any order, duplicates allowed;
    ``row_begin`` / ``rows`` / ``doy`` / ``windows`` / ``checked`` as for :func:`spell_reduce`.  There is no workspace: a window
    does not add across the parts of a list, so a period's list is never split.  Returns ``(out, status)``: the (n_win, P, n)
    tensor and the status word (bit 0: an in-season value was +-inf)."""
    X = _check_X(X, "TG")
    try:
        raw = list(np.atleast_1d(np.asarray(lengths, dtype=object)))
    except (TypeError, ValueError):
        raise ValueError("lengths must be a sequence of integers, got %r" % (lengths,)) from None
    if not 1 <= len(raw) <= _lib.ROLL_MAX_WINDOWS:
        raise ValueError("1..%d window lengths per call, got %d" % (_lib.ROLL_MAX_WINDOWS, len(raw)))
    for w in raw:
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, np.integer)) or not 1 <= w <= _lib.ROLL_WINDOW_MAX:
            raise ValueError("a window length must be an integer in 1..%d, got %r" % (_lib.ROLL_WINDOW_MAX, w))
    if stat not in _ROLL_STATS:
        raise ValueError("stat must be 'max' or 'min', got %r" % (stat,))
    if of not in _ROLL_OF:
        raise ValueError("of must be 'mean' or 'sum', got %r" % (of,))
    w32 = np.ascontiguousarray([int(w) for w in raw], dtype=np.int32)
    return _grouped_reduce("wagg_rolling_reduce", (X,), row_begin, rows, doy, windows, checked, offset,
                           (_np_ptr(w32, C.c_int32), len(w32), _ROLL_STATS[stat], _ROLL_OF[of]), len(w32),
                           lambda L, *a: L.wagg_rolling_work_bytes(*a), out, status, False, stream)


_QUANT_METHODS = {"linear": _lib.QUANT_LINEAR, "lower": _lib.QUANT_LOWER, "higher": _lib.QUANT_HIGHER}


def _quantile_levels(q):
    """``q`` as a float64 vector in the caller's order: 1 .. ``_lib.QUANT_MAX`` finite numbers in [0, 1] (no bool) -- else ValueError"""
    try:
        raw = list(np.atleast_1d(np.asarray(q, dtype=object)))
    except (TypeError, ValueError):
        raise ValueError("q must be a sequence of numbers in [0, 1], got %r" % (q,)) from None
    if not 1 <= len(raw) <= _lib.QUANT_MAX:
        raise ValueError("1..%d quantiles per call, got %d" % (_lib.QUANT_MAX, len(raw)))
    for v in raw:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError("a quantile must be a finite number in [0, 1], got %r" % (v,))
    return np.ascontiguousarray([float(v) for v in raw], dtype=np.float64)


def quantile_select(X, row_begin, rows, offset, q, method="linear", max_rows=None, doy=None, windows=None, checked=False, out=None,
                    status=None, stream=None):
    """Per-cell quantiles of the daily values of every period, for every level of ``q`` in ONE launch
    (``wagg_quantile_select_*``).  Entry ``i`` of period ``p``'s list is valid for cell ``j`` when its row ``t`` lies in the
    field, the cell is in season on ``doy[t]`` and ``X[t, j]`` is not NaN; order and gaps do not matter, a row listed twice
    counts twice, an in-season +-inf is valid.  With ``m`` valid entries and ``v[0] <= ... <= v[m - 1]`` their raw elements
    sorted: ``h = (m - 1) * q[k]`` in fp64, ``lo = floor(h)``, ``g = h - lo``; ``method="linear"``: ``v[lo] + (v[lo + 1] - v[lo])
    * g`` in fp64 without a fused multiply-add (``v[lo]`` itself where ``g == 0``), ``"lower"``: ``v[lo]``, ``"higher"``:
    ``v[lo + 1]`` (``v[lo]`` where ``g == 0``).  ``out[k, p, j]`` is that plus ``offset``, rounded once to ``X``'s dtype, and NaN
    where the period holds no valid entry for the cell.  ``X``: a (T, n) CUDA tensor; ``q``: 1 .. ``_lib.QUANT_MAX`` finite
    numbers in [0, 1] in any order, duplicates allowed (a bool, a NaN or a value outside is ValueError); ``row_begin`` / ``rows``
    / ``doy`` / ``windows`` / ``checked`` as for :func:`rolling_reduce`.  ``max_rows``: the caller's bound on the longest list, 1
    .. ``_lib.QUANT_ROWS_MAX`` -- a block holds its period's whole list in 128 * ``max_rows`` bytes of LDS; None takes the
    longest list itself: from host integers at no cost, FROM DEVICE LISTS WITH ONE ``row_begin.diff().max()`` THAT BLOCKS.  A
    list longer than ``max_rows`` is an error of the library's look at the lists; with ``checked=True`` (no look) the kernel
    writes NaN for that period and sets bit 1 of the status word.  There is no workspace: a list is never split.  ``stream=``
    as for :func:`rolling_reduce`: the kernel, the zero-fill of ``status`` and the tensors allocated here are ordered on it --
    but the ``row_begin.diff().max()`` of ``max_rows=None`` on device lists runs on torch's CURRENT stream and blocks, so a
    caller who wants a non-blocking call on ``stream`` passes ``max_rows``.
    Returns ``(out, status)``: the (n_q, P, n) tensor and the status word (bit 0: an in-season value was +-inf; bit 1: a list
    was longer than ``max_rows``)."""
    import torch
    X = _check_X(X, "TG")
    qv = _quantile_levels(q)
    if method not in _QUANT_METHODS:
        raise ValueError("method must be 'linear', 'lower' or 'higher', got %r" % (method,))
    if max_rows is None:
        if isinstance(row_begin, torch.Tensor):
            longest = int(row_begin.diff().max().item()) if row_begin.numel() > 1 else 0        # (blocks)
        else:
            rb = np.asarray(row_begin, dtype=np.int64)
            longest = int(np.diff(rb).max()) if rb.ndim == 1 and len(rb) > 1 else 0
        if longest > _lib.QUANT_ROWS_MAX:
            raise ValueError("a period lists %d rows; a quantile call holds at most %d" % (longest, _lib.QUANT_ROWS_MAX))
        max_rows = max(1, longest)
    if isinstance(max_rows, (bool, np.bool_)) or not isinstance(max_rows, (int, np.integer)) or not 1 <= max_rows <= _lib.QUANT_ROWS_MAX:
        raise ValueError("max_rows must be an integer in 1..%d, got %r" % (_lib.QUANT_ROWS_MAX, max_rows))
    return _grouped_reduce("wagg_quantile_select", (X,), row_begin, rows, doy, windows, checked, offset,
                           (_np_ptr(qv, C.c_double), len(qv), _QUANT_METHODS[method], int(max_rows)), len(qv),
                           lambda L, *a: 0, out, status, False, stream)


def hinge_reduce(X, row_begin, rows, offset, knots, power=1, side="above", tail=None, doy=None, windows=None, checked=False, out=None,
                 status=None, workspace=None, stream=None):
    """Truncated powers of a field about every knot of a list, summed per period, in ONE launch (``wagg_hinge_reduce_*``):
    ``out[j, p, i]`` sums ``max(+-((X[t, i] + offset) - knots[j]), 0) ** power`` over the rows ``t`` of period ``p`` on which
    cell ``i`` is in season; ``+`` for ``side="above"``, ``-`` for ``"below"``.  ``X``: a (T, n) CUDA tensor; ``knots``:
    1 .. ``_lib.HINGE_MAX`` finite numbers in any order (the kernel takes them ``_lib.HINGE_GROUP`` at a time); ``power``: 1, 2
    or 3; ``row_begin`` / ``rows`` / ``doy`` / ``windows`` / ``checked`` / ``workspace`` as for :func:`bin_days_reduce`.
    ``tail=(tail_knots, a, b)``: two more knots and a coefficient pair per plane; plane ``j`` is then ``S_j + a[j] * S_A +
    b[j] * S_B`` with the same sums at the tail knots, combined in fp64 before the cast (the restricted cubic spline).
    The difference is formed in ``X``'s dtype, in the two roundings written above; powers are products in that dtype; sums are
    fp64.  NaN counts 0.  Returns ``(planes, status)``: the (n_knots, P, n) tensor of ``X``'s dtype and the status word (bit 0:
    an in-season value of the field was +-inf)."""
    X = _check_X(X, "TG")
    k = np.ascontiguousarray(np.atleast_1d(knots), dtype=np.float64)
    if k.ndim != 1 or not 1 <= len(k) <= _lib.HINGE_MAX:
        raise ValueError("1..%d knots per call, got %s" % (_lib.HINGE_MAX, k.shape))
    if not np.isfinite(k).all():
        raise ValueError("knots must be finite, got %r" % (k.tolist(),))
    if power not in (1, 2, 3):
        raise ValueError("power must be 1, 2 or 3, got %r" % (power,))
    _check_side(side)
    tk = ta = tb = None
    if tail is not None:
        tk, ta, tb = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in tail)
        if tk.shape != (2,) or ta.shape != k.shape or tb.shape != k.shape or not all(np.isfinite(v).all() for v in (tk, ta, tb)):
            raise ValueError("tail must be (two knots, a coefficient per knot, a coefficient per knot), all finite")
    dptr = lambda v: None if v is None else _np_ptr(v, C.c_double)
    return _grouped_reduce("wagg_hinge_reduce", (X,), row_begin, rows, doy, windows, checked, offset,
                           (dptr(k), len(k), int(power), _lib.HINGE_ABOVE if side == "above" else _lib.HINGE_BELOW, dptr(tk),
                            dptr(ta), dptr(tb)), len(k), lambda L, *a: L.wagg_hinge_work_bytes(*a), out, status,
                           True if workspace is None else workspace, stream)


def season_mask(doy, windows, stream=None):
    """The growing-season mask itself (``wagg_season_mask``): a float64 (n, T) CUDA tensor, 1 where cell ``j`` is in season on
    the day of year ``doy[t]``, 0 where it is not, NaN for a null window.  ``doy`` / ``windows`` as for :func:`season_reduce`."""
    torch = require_gpu()
    dev = next((a.device for a in (doy, windows) if isinstance(a, torch.Tensor)), "cuda")
    doy = _season_vector(doy, len(doy), "doy", dev)
    windows = _season_vector(windows, len(windows), "windows", dev)
    if doy.device != windows.device:
        raise ValueError("doy and windows must live on one device")
    with _on_stream(stream):
        out = torch.empty((int(windows.numel()), int(doy.numel())), dtype=torch.float64, device=doy.device)
    _lib.check(_lib.load().wagg_season_mask(C.c_void_p(doy.data_ptr()), int(doy.numel()), C.c_void_p(windows.data_ptr()),
                                            int(windows.numel()), C.c_void_p(out.data_ptr()), _stream_handle(stream)), "wagg_season_mask")
    if stream is not None:
        doy.record_stream(stream)
        windows.record_stream(stream)
    return out


def take_axis(t, axis, index, stream=None):
    """``t`` with only the positions ``index`` (host integers) kept / re-ordered along ``axis`` (``wagg_take_axis``):
    the leap-day drop and the lon re-ordering of a device-resident field, without a torch kernel.  The index is uploaded by a
    blocking copy on torch's CURRENT stream (so the call waits for what is queued there); everything else runs on ``stream``,
    to which the result then belongs in torch's allocator (the module's docstring)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError("expected a torch tensor")
    axis = int(axis) % t.dim()
    idx = np.ascontiguousarray(index, dtype=np.int64)
    if len(idx) and (idx.min() < 0 or idx.max() >= t.shape[axis]):
        raise IndexError("index out of range")
    if not t.is_cuda:                                # host tensor: a host copy, nothing for the device to do
        return torch.from_numpy(np.take(t.numpy(), idx, axis=axis))
    if t.dtype not in (torch.float32, torch.float64):
        t = to_float64(t, stream=stream)             # (rows of 1- and 2-byte elements are not whole words: promote first, S8)
    t = relayout(t, stream=stream) if not t.is_contiguous() else t
    outer = int(np.prod(t.shape[:axis], dtype=np.int64))
    inner_bytes = int(np.prod(t.shape[axis + 1:], dtype=np.int64)) * t.element_size()
    with _on_stream(stream):
        out = torch.empty(tuple(t.shape[:axis]) + (len(idx),) + tuple(t.shape[axis + 1:]), dtype=t.dtype, device=t.device)
    idx_dev = torch.from_numpy(idx).to(t.device)
    _lib.check(_lib.load().wagg_take_axis(C.c_void_p(t.data_ptr()), outer, int(t.shape[axis]), inner_bytes,
                                          C.c_void_p(idx_dev.data_ptr()), len(idx), C.c_void_p(out.data_ptr()),
                                          _stream_handle(stream)), "wagg_take_axis")
    if stream is not None:                           # idx_dev goes back to torch's allocator on return: keep it alive until
        idx_dev.record_stream(stream)                # the kernel on the caller's stream has read it
    return out


def upload(a):
    """A C-contiguous float32 / float64 NumPy array as a CUDA tensor of the current device (``wagg_upload``: page-locked in
    place for one DMA when it is large, through the library's staging pieces otherwise; blocking)."""
    torch = require_gpu()
    a = np.ascontiguousarray(a)
    dt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}.get(a.dtype)
    if dt is None:
        raise TypeError("float32 or float64 arrays only, got %s" % a.dtype)
    out = torch.empty(a.shape, dtype=dt, device="cuda")
    torch.cuda.current_stream().synchronize()          # (the caching allocator may hand out memory the stream still writes)
    _lib.check(_lib.load().wagg_upload(C.c_void_p(out.data_ptr()), C.c_void_p(a.ctypes.data), a.nbytes), "wagg_upload")
    return out


def relayout(t, order=None, stream=None):
    """A contiguous copy of ``t`` (float32/float64 CUDA tensor, any strides), its dims in ``order`` if given
    (``wagg_relayout_*``): what ``permute(order).contiguous()`` would do, in the library's own kernel.  With ``stream=`` the
    copy belongs to that stream in torch's allocator (the module's docstring; the same for :func:`to_float64` and the
    ``transform_*`` / :func:`combine_planes` results)."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.float32, torch.float64)):
        raise TypeError("device-resident fields must be float32 or float64 CUDA tensors, got %s" % getattr(t, "dtype", type(t)))
    order = list(range(t.dim())) if order is None else [int(i) for i in order]
    if t.dim() > 6 or t.dim() < 1:
        raise ValueError("1..6 dimensions")
    shape = [int(t.shape[i]) for i in order]
    strides = [int(t.stride(i)) for i in order]
    with _on_stream(stream):
        out = torch.empty(shape, dtype=t.dtype, device=t.device)
    sh = (C.c_int64 * len(shape))(*shape)
    st = (C.c_int64 * len(shape))(*strides)
    L = _lib.load()
    fn = L.wagg_relayout_f32 if t.dtype == torch.float32 else L.wagg_relayout_f64
    _lib.check(fn(C.c_void_p(t.data_ptr()), len(shape), sh, st, C.c_void_p(out.data_ptr()), _stream_handle(stream)), "wagg_relayout")
    return out


_TO_F64_TYPES = {"torch.float16": 0, "torch.bfloat16": 1, "torch.int8": 2, "torch.uint8": 3, "torch.int16": 4, "torch.int32": 5,
                 "torch.int64": 6, "torch.float32": 7, "torch.float64": 8}


def to_float64(t, order=None, stream=None):
    """A contiguous float64 copy of a CUDA tensor of another dtype (any strides; dims in ``order`` if given), converted in
    the library's own kernel (``wagg_relayout_to_f64``) -- the reference's promotion: data times float64 weights is float64."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError("expected a CUDA tensor")
    code = _TO_F64_TYPES.get(str(t.dtype))
    if code is None:
        raise TypeError("device-resident fields of dtype %s are not supported" % (t.dtype,))
    order = list(range(t.dim())) if order is None else [int(i) for i in order]
    if t.dim() > 6 or t.dim() < 1:
        raise ValueError("1..6 dimensions")
    shape = [int(t.shape[i]) for i in order]
    strides = [int(t.stride(i)) for i in order]
    with _on_stream(stream):
        out = torch.empty(shape, dtype=torch.float64, device=t.device)
    sh = (C.c_int64 * len(shape))(*shape)
    st = (C.c_int64 * len(shape))(*strides)
    _lib.check(_lib.load().wagg_relayout_to_f64(C.c_void_p(t.data_ptr()), code, len(shape), sh, st, C.c_void_p(out.data_ptr()),
                                                _stream_handle(stream)), "wagg_relayout_to_f64")
    return out


def any_less(a, b, stream=None):
    """True iff some a[i] < b[i] (``wagg_any_less_*``: the tasmax < tasmin check of
    transformations.py:62); blocks."""
    import torch
    a, b = _flat_dev(a, stream), _flat_dev(b, stream)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("operands must have the same shape and dtype")
    res = C.c_int(0)
    L = _lib.load()
    fn = L.wagg_any_less_f32 if a.dtype == torch.float32 else L.wagg_any_less_f64
    _lib.check(fn(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.numel(), C.byref(res), _stream_handle(stream)),
               "wagg_any_less")
    return bool(res.value)


def to_device(values):
    """NumPy array (one pageable H2D copy) or CUDA tensor (as it is) -> CUDA tensor."""
    import torch
    if isinstance(values, torch.Tensor):
        return values if values.is_cuda else values.cuda()
    return torch.from_numpy(np.ascontiguousarray(values)).cuda()


def synth_field(T, G, seed, base, amp, dtype="float32", device="cuda"):
    """X[t, g] = base + amp * (hash_u01(t*G + g, seed) - 0.5), generated on the device."""
    torch = require_gpu()
    dt = torch.float32 if dtype in ("float32", torch.float32) else torch.float64
    X = torch.empty((T, G), dtype=dt, device=device)
    L = _lib.load()
    fn = L.wagg_synth_field_f32 if dt == torch.float32 else L.wagg_synth_field_f64
    _lib.check(fn(C.c_void_p(X.data_ptr()), T, G, G, int(seed), base, amp, _stream_handle(None)),
               "wagg_synth_field")
    return X


def synth_table_csr(G, R, seed, fill, blocklocal=False):
    """The c5 weight tables of :meth:`DensePlan.synth` / :meth:`DensePlan.synth_blocklocal` as host CSR arrays
    ``(rowptr int64, col int32, val float64)`` -- what a caller with a real table would hand to
    :meth:`DensePlan.from_csr` (``wagg_synth_table_csr``: generated on the device, copied out)."""
    require_gpu()
    L = _lib.load()
    rowptr = np.empty(int(G) + 1, dtype=np.int64)
    nnz = C.c_int64(0)
    args = (int(G), int(R), int(seed), float(fill), 1 if blocklocal else 0, _np_ptr(rowptr, C.c_int64))
    _lib.check(L.wagg_synth_table_csr(*args, None, None, 0, C.byref(nnz)), "wagg_synth_table_csr")
    col = np.empty(nnz.value, dtype=np.int32)
    val = np.empty(nnz.value, dtype=np.float64)
    _lib.check(L.wagg_synth_table_csr(*args, _np_ptr(col, C.c_int32), _np_ptr(val, C.c_double), nnz.value, C.byref(nnz)),
               "wagg_synth_table_csr")
    return rowptr, col, val


def profile_enable(on=True):
    """Record HIP event pairs around the dominant kernel of every following apply."""
    _lib.check(_lib.load().wagg_profile_enable(1 if on else 0), "wagg_profile_enable")


PROFILE_SLOTS = 1024      # wagg.h WAGG_PROFILE_SLOTS


def profile_read():
    """Durations (ms) of the dominant kernels recorded since profile_enable(); blocks."""
    buf = (C.c_float * PROFILE_SLOTS)()
    n = C.c_int(0)
    _lib.check(_lib.load().wagg_profile_read(buf, PROFILE_SLOTS, C.byref(n)), "wagg_profile_read")
    return [float(buf[i]) for i in range(n.value)]


def profile_event_overhead(n=64, stream=None):
    """(median, minimum) milliseconds that an event pair handed to the launch of an EMPTY kernel reads
    (``wagg_profile_event_overhead``): the floor under every ``profile_read`` figure."""
    med, mn = C.c_float(0.0), C.c_float(0.0)
    _lib.check(_lib.load().wagg_profile_event_overhead(_stream_handle(stream), int(n), C.byref(med), C.byref(mn)),
               "wagg_profile_event_overhead")
    return float(med.value), float(mn.value)
