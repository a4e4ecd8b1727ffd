"""Builds tests/chunk_dump.cpp (the stand-alone dump of the host chunking stages) with the host compiler; plans from its
tables through the C-ABI."""
import ctypes as C
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("32x8", "16x8", "16x4")


def build_dump(outdir, target="chunk_dump"):
    """`make <target>` (chunk_dump or chunk_dump_san) into `outdir`; returns the program's path."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "climate_toolbox_amd", "csrc"), target, "CHUNK_OUT=" + str(outdir)])
    return os.path.join(str(outdir), target)


def run_dump(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return r.stdout


def dump_tables(program):
    """The dump program's built-in tables that have at least one row, as numpy arrays."""
    import numpy as np
    out = []
    for t in json.loads(run_dump(program, "--tables")):
        if t["cell"]:
            out.append(dict(t, cell=np.asarray(t["cell"], np.int32), region=np.asarray(t["region"], np.int32),
                            w=np.asarray(t["w"], np.float64)))
    return out


def plan_record(L, t, flags):
    """wagg_plan_create over table `t`: every field of wagg_plan_get_info and wagg_plan_get_den (as float.hex strings)."""
    import numpy as np
    from climate_toolbox_amd import _lib
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    plan = C.c_void_p()
    rc = L.wagg_plan_create(t["cell"].ctypes.data_as(i32p), t["region"].ctypes.data_as(i32p), t["w"].ctypes.data_as(f64p),
                            len(t["cell"]), t["G"], t["R"], t["row_len"], flags, C.byref(plan))
    assert rc == 0, (t["name"], flags, rc, L.wagg_last_error())
    try:
        info = _lib.PlanInfo()
        assert L.wagg_plan_get_info(plan, C.byref(info)) == 0
        den = np.full(t["R"], np.nan)
        assert L.wagg_plan_get_den(plan, den.ctypes.data_as(f64p)) == 0
    finally:
        L.wagg_plan_destroy(plan)
    rec = {k: int(getattr(info, k)) for k, _ in _lib.PlanInfo._fields_}
    rec["den"] = [float(x).hex() for x in den]
    return rec
