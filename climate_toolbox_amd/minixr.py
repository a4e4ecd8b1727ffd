"""A very small labelled-array container used when ``xarray`` is not importable.

It exists only so that the drop-in functions of ``climate_toolbox_amd.aggregations`` have an
object to take and return in an environment without xarray (this image has none).  It models the
handful of attributes the reference path touches (aggregations.py:24-27, :64-82 and
tests/test_climate_toolbox.py:51-64,109-135): ``Dataset(data_vars, coords)``, ``ds[name]``,
``ds.name``, ``ds.dims``, ``ds.coords``, ``DataArray.values/.dims/.shape/.isnull()/.any()``.
It is NOT an xarray re-implementation and carries no arithmetic.
"""
from __future__ import annotations

import numpy as np


class DataArray:
    def __init__(self, values, dims=None, coords=None, name=None):
        self._values = values if hasattr(values, "shape") else np.asarray(values)
        if dims is None:
            dims = tuple("dim_%d" % i for i in range(self._values.ndim))
        if isinstance(dims, str):
            dims = (dims,)
        self.dims = tuple(dims)                       # iterating a dict yields its keys (ref :65)
        if len(self.dims) != self._values.ndim:
            raise ValueError("dims %r do not match array of shape %r" % (self.dims, self._values.shape))
        self.coords = dict(coords or {})
        self.name = name
        self.attrs = {}

    @property
    def values(self):
        v = self._values
        if type(v).__module__.startswith("torch"):      # a device-resident buffer: copy out on demand
            return v.detach().cpu().numpy()
        return np.asarray(v)

    @property
    def data(self):
        """The buffer as it is held (xarray's ``.data``): a NumPy array, or a torch CUDA tensor for device-resident
        variables and for results returned under ``results_on_device()`` -- no copy."""
        return self._values

    @property
    def shape(self):
        return tuple(self._values.shape)

    @property
    def dtype(self):
        return self._values.dtype

    @property
    def ndim(self):
        return self._values.ndim

    @property
    def sizes(self):
        return dict(zip(self.dims, self.shape))

    def __len__(self):
        return self.shape[0]

    def __iter__(self):
        return iter(self.values)

    def isnull(self):
        v = self.values
        if v.dtype.kind == "f":
            return DataArray(np.isnan(v), self.dims)
        if v.dtype == object:
            return DataArray(np.array([x is None or x != x for x in v.ravel()]).reshape(v.shape), self.dims)
        return DataArray(np.zeros(v.shape, dtype=bool), self.dims)

    def notnull(self):
        return DataArray(~self.isnull().values, self.dims)

    def any(self):
        return bool(np.any(self.values))

    def all(self):
        return bool(np.all(self.values))

    def __bool__(self):
        return bool(self.values)

    def __array__(self, dtype=None, copy=None):
        v = self.values
        return v.astype(dtype) if dtype is not None else v

    def __repr__(self):
        return "<minixr.DataArray %s %r %s>" % (self.name or "", dict(zip(self.dims, self.shape)), self.dtype)


class LazyArray(DataArray):
    """A data variable that keeps the buffer it was loaded with and carries, instead of a copy,
    (a) a re-ordering of its ``lon`` axis (element j along ``lon`` is column ``lon_perm[j]`` of
    the buffer; standardize.py) and/or (b) an element transform ``(x + offset) ** power``
    (transformations.py).  The aggregation folds (a) into the plan's cell index and evaluates (b)
    while the data is loaded on the GPU; ``.values`` materialises the array on demand."""

    def __init__(self, raw, dims, lon_perm=None, xform=None, name=None, attrs=None, edd=None):
        super().__init__(raw, dims, name=name)
        self._lon_perm = None if lon_perm is None else np.asarray(lon_perm, dtype=np.int64)
        self._xform = None if xform is None else (float(xform[0]), int(xform[1]))
        # (c) Snyder degree days of (tasmin = this buffer, tasmax = edd[0]) shifted by edd[1]:
        # sum of coef * EDD(threshold) over edd[2] = [(coef, threshold), ...]  (transformations.py)
        self._edd = None if edd is None else (edd[0], float(edd[1]), [(float(c), float(e)) for c, e in edd[2]])
        self.attrs = dict(attrs or {})

    def _replace(self, raw=None, dims=None, edd_raw=None, **over):
        """Copy of this variable with another buffer / dims, keeping the lon permutation, the lazy
        transform, the degree-day partner and the attrs (``edd_raw`` = the tasmax buffer after the
        same edit as ``raw``; a lazy degree-day variable cannot be re-built without it)."""
        edd = self._edd
        if edd is not None and raw is not None:
            if edd_raw is None:
                raise ValueError("a lazy degree-day variable needs both of its buffers edited alike")
            edd = (edd_raw, edd[1], edd[2])
        kw = dict(lon_perm=self._lon_perm, xform=self._xform, name=self.name, attrs=self.attrs, edd=edd)
        kw.update(over)
        return LazyArray(self._values if raw is None else raw, self.dims if dims is None else dims, **kw)

    def _ordered(self, buf):
        """``buf`` (host array or device tensor, file order) with the lon permutation applied."""
        if self._lon_perm is None or "lon" not in self.dims:
            return buf
        ax = self.dims.index("lon")
        if _is_tensor(buf):
            from . import engine
            return engine.take_axis(buf, ax, self._lon_perm)          # wagg_take_axis
        return np.take(np.asarray(buf), self._lon_perm, axis=ax)

    @property
    def values(self):
        raw = self._ordered(self._values)
        if self._xform is None and self._edd is None:
            return raw.detach().cpu().numpy() if _is_tensor(raw) else np.asarray(raw)
        # transforms are evaluated on the device by the kernels' own device functions
        # (wagg_transform_*), never on the host
        from . import engine
        engine.require_gpu()
        t = engine.to_device(raw)
        if self._xform is not None:
            off, pw = self._xform
            t = engine.transform_poly(t, off, pw)
        if self._edd is not None:
            hi, off, terms = self._edd
            t = engine.transform_edd(t, engine.to_device(self._ordered(hi)), off, terms)
        return t.cpu().numpy()


def _is_tensor(v):
    return type(v).__module__.startswith("torch")


class _Coords(dict):
    def __init__(self, owner):
        super().__init__()
        self._owner = owner

    def __setitem__(self, key, value):
        super().__setitem__(key, self._owner._as_array(key, value))


class Dataset:
    def __init__(self, data_vars=None, coords=None):
        self.coords = _Coords(self)
        self.data_vars = {}
        for k, v in (coords or {}).items():
            self.coords[k] = v
        for k, v in (data_vars or {}).items():
            self[k] = v

    def _as_array(self, key, value):
        if isinstance(value, DataArray):
            value.name = key
            return value
        if isinstance(value, tuple) and len(value) >= 2 and not hasattr(value, "shape"):
            dims, vals = value[0], value[1]
            return DataArray(np.asarray(vals) if not hasattr(vals, "shape") else vals, dims, name=key)
        arr = np.asarray(value)
        return DataArray(arr, (key,) if arr.ndim == 1 else None, name=key)

    @property
    def dims(self):
        out = {}
        for arr in list(self.data_vars.values()) + list(self.coords.values()):
            for d, n in zip(arr.dims, arr.shape):
                out.setdefault(d, n)
        return out

    sizes = dims

    def __getitem__(self, key):
        if key in self.data_vars:
            return self.data_vars[key]
        if key in self.coords:
            return self.coords[key]
        raise KeyError(key)

    def __setitem__(self, key, value):
        self.data_vars[key] = self._as_array(key, value)

    def __contains__(self, key):
        return key in self.data_vars or key in self.coords

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __repr__(self):
        return "<minixr.Dataset dims=%r vars=%r coords=%r>" % (
            self.dims, list(self.data_vars), list(self.coords))
