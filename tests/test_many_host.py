"""Many-plans (wagg_plan_create_many) without a GPU: the builder's checks refuse bad input before any device call, valid
input gets as far as the device, the nesting helper groups levels, and the builder runs under ASan / UBSan."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from climate_toolbox_amd import _lib, synth
from climate_toolbox_amd.engine import _many_args
from climate_toolbox_amd.many import nest_map, nesting_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(ci, rc, ws, G, R, levels=(), row_len=0):
    L = _lib.load()
    keep, head, tail = _many_args(ci, rc, ws, levels)
    h = C.c_void_p()
    st = L.wagg_plan_create_many(*head, int(G), int(R), int(row_len), tail[0], tail[1], tail[2], 0, C.byref(h))
    msg = L.wagg_last_error().decode()
    if st == 0:
        L.wagg_plan_destroy(h)
    del keep
    return st, msg


def _table(n=2000, G=4096, R=50, seed=0):
    rng = np.random.default_rng(seed)
    ci = rng.integers(0, G, n).astype(np.int32)
    rc = rng.integers(0, R, n).astype(np.int32)
    iso = (rc // 10).astype(np.int32)                      # nests: 5 coarse regions
    return ci, rc, iso, rng.uniform(0.1, 1, n), rng.uniform(0.1, 1, n)


def test_many_entry_points_exported():
    L = _lib.load()
    for name in ("wagg_plan_create_many", "wagg_plan_many_info", "wagg_plan_get_den_many"):
        getattr(L, name)
    assert L.wagg_version() >= 500


def test_bad_weight_counts_and_columns():
    L = _lib.load()
    ci, rc, iso, a, p = _table()
    assert _create(ci, rc, [], 4096, 50)[0] == -1
    st, msg = _create(ci, rc, [a, p, a, p, a], 4096, 50)
    assert st == -1 and "n_weights" in msg
    keep, head, tail = _many_args(ci, rc, [a, p], ())
    wp = (C.POINTER(C.c_double) * 2)(head[2][0], C.POINTER(C.c_double)())
    h = C.c_void_p()
    assert L.wagg_plan_create_many(head[0], head[1], wp, 2, head[4], 4096, 50, 0, tail[0], tail[1], 0, 0, C.byref(h)) == -1
    assert "weight column 1 is NULL" in L.wagg_last_error().decode()


def test_level_code_out_of_range():
    ci, rc, iso, a, p = _table()
    bad = iso.copy(); bad[17] = 5
    st, msg = _create(ci, rc, [a, p], 4096, 50, [(bad, 5)])
    assert st == -1 and "[17]" in msg and "out of range" in msg


def test_level_that_does_not_nest_names_the_row():
    ci, rc, iso, a, p = _table()
    bad = iso.copy()
    rows = np.nonzero(rc == rc[300])[0]
    bad[rows[-1]] = (bad[rows[-1]] + 1) % 5                # one fine region split over two coarse ones
    st, msg = _create(ci, rc, [a, p], 4096, 50, [(bad, 5)])
    assert st == -1 and "does not nest" in msg and ("row %d " % rows[-1]) in msg


def test_null_fine_label_with_a_coarse_label():
    ci, rc, iso, a, p = _table()
    rc2 = rc.copy(); rc2[40] = -1
    st, msg = _create(ci, rc2, [a, p], 4096, 50, [(iso, 5)])
    assert st == -1 and "row 40 " in msg and "null on one level only" in msg


def test_valid_input_reaches_the_device():
    ci, rc, iso, a, p = _table()
    a2 = a.copy(); a2[::7] = np.nan                        # kept rows diverge: popwt keeps them
    st, msg = _create(ci, rc, [p, a2], 4096, 50, [(iso, 5)], row_len=64)
    assert st in (0, -2, -4), (st, msg)
    st, msg = _create(ci, rc, [a], 4096, 50)
    assert st in (0, -2, -4), (st, msg)


def test_nesting_helper_on_realistic_labels():
    lat, lon, df = synth.realistic_segments(nlat=90, nlon=180, R=300, n_iso=20, seed=3, string_labels=True)
    _, hier = np.unique(df["hierid"].values.astype(str), return_inverse=True)
    _, iso = np.unique(df["ISO"].values.astype(str), return_inverse=True)
    m = nest_map(hier, iso)
    assert m is not None and (m[hier] == iso).all()
    assert nest_map(iso, hier) is None
    assert nesting_order({"ISO": iso, "hierid": hier}) == [("hierid", ["ISO"])]
    other = np.random.default_rng(1).integers(0, 7, len(hier))      # a grouping that cuts across the regions
    assert nest_map(hier, other) is None
    assert nesting_order({"hierid": hier, "ISO": iso, "zone": other}) == [("hierid", ["ISO"]), ("zone", [])]
    nulled = iso.copy(); nulled[5] = -1
    assert nest_map(hier, nulled) is None


def test_many_builder_is_clean_under_asan_ubsan():
    rt = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so")
    if not rt:
        pytest.skip("clang AddressSanitizer runtime not found")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "climate_toolbox_amd", "csrc"), "hostsan"])
    env = dict(os.environ, LD_PRELOAD=rt[0], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hostsan_many_check.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "hostsan many ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_nest_map_follows_the_builders_kept_rows():
    fine = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    coarse = np.array([0, 0, 1, 0, 1], dtype=np.int32)          # fine region 1 meets two coarse ones ...
    assert nest_map(fine, coarse) is None
    kept = np.array([True, True, True, False, True])             # ... but only on a row no weighting keeps
    np.testing.assert_array_equal(nest_map(fine, coarse, kept), [0, 1, 1])
    assert nesting_order({"f": fine, "c": coarse}, kept) == [("f", ["c"])]


def test_dataset_function_is_exported():
    import climate_toolbox_amd as P
    from climate_toolbox_amd import many
    assert P.weighted_aggregate_grid_to_regions_many is many.weighted_aggregate_grid_to_regions_many
