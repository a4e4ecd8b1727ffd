"""The device plan builder (csrc/wagg_build.hip) at the edges of its sort, scans and runs: every stored weight of a plan
against the fp64 restatement of tests/build_tables.py, read back with an impulse probe (row t of X holds one power of two in
one cell: out[t, r] den[r] is the stored weight of (cell, r)).

Tolerances (none measured): a stored weight within 2^-51 (fp64) / 2^-22 (fp32) of the TABLE-ORDER pair sum, an exact 0 where
that sum is 0 or no pair exists, NaN / +-inf where den == 0; nnz and info["one_pass_sort"] exact; den[r] within
n_r 2^-53 sum |pair sum| of math.fsum.  Bit equality (den, the probe, a random 17-row field) between COO and CSR of one
table, between the one-pass route and general_sort=True, between two builds, and -- tables without repeated pairs -- between
row permutations.  Repeated pairs carry order-sensitive weights (A, b, -A, c with A = 2^60: see tests/build_tables.py), in
COO tables scattered over rounds, wave slices and sort tiles of the radix sort.

The cases are numbered as in the functions' names; tests/test_build_tables_host.py checks the tables, the restatement and
the comparison (that it fails on a swapped, lost, displaced or split row) without a GPU."""
import functools

import numpy as np
import pytest

from tests import build_tables as B
from tests.test_gpu_parity import torch_cuda  # noqa: F401  (the parity tests' fixture)

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FORM_CODE = {"full": 0, "tiles": 1, "entries": 2}
ALL_FORMS = ("full", "entries", "tiles")


# ---- shared, unchanged inputs --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(maker, *args):
    return getattr(B, maker)(*args)


@functools.lru_cache(maxsize=8)
def routes_of(t):
    """{route: (constructor name, arrays)} of one table; the CSR orders are computed once"""
    return {"coo": ("from_segments", t.coo()), "csr": ("from_csr", t.csr()), "csr_sorted": ("from_csr", t.csr(sort_columns=True))}


class _Dev:
    """the probe and the 17-row field of a table on the device, kept while the table's routes and forms are walked"""
    def __init__(self, torch, t, dtype):
        self.torch, self.t = torch, t
        self.cells = B.probe_cells(t)
        td = torch.float64 if dtype == F64 else torch.float32
        X = torch.zeros((len(self.cells), t.G), dtype=td, device="cuda")
        X[torch.arange(len(self.cells), device="cuda"), torch.from_numpy(self.cells).cuda()] = torch.from_numpy(
            B.amplitudes(self.cells).astype(dtype)).cuda()
        self.X = X
        self.field = torch.from_numpy(np.random.default_rng(t.G + t.R).standard_normal((17, t.G)).astype(dtype)).cuda()


class _Read:
    pass


def build(t, route, form, dtype, general_sort=False):
    from climate_toolbox_amd.engine import DensePlan
    ctor, arrays = routes_of(t)[route]
    kw = dict(general_sort=True) if general_sort else {}
    plan = getattr(DensePlan, ctor)(*arrays, t.G, t.R, dtype=dtype, form=form, **kw)
    assert plan.info["form"] == FORM_CODE[form] and plan.dtype == np.dtype(dtype).name
    if ctor == "from_csr":
        assert plan.info["one_pass_sort"] == t.expect_one_pass(arrays[0], arrays[1], general_sort), (t.name, route, general_sort)
    else:
        assert plan.info["one_pass_sort"] == 0
    return plan


def read(dev, t, route, form, dtype, general_sort=False):
    """build, probe, apply the 17-row field, close"""
    plan = build(t, route, form, dtype, general_sort)
    try:
        r = _Read()
        exact = dtype == F32 and form == "full"                  # the fp32 full form: the exact kernel, not the split one
        r.probe = plan.apply(dev.X, exact=exact).cpu().numpy()
        r.applied = plan.apply(dev.field, exact=exact).cpu().numpy()
        r.den, r.nnz, r.one_pass = plan.den.copy(), plan.info["nnz"], plan.info["one_pass_sort"]
        return r
    finally:
        plan.close()


def same_bits(a, b, what):
    for name in ("den", "probe", "applied"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg="%s: %s" % (what, name))
    assert a.nnz == b.nnz, what


def walk(torch, t, routes, forms=ALL_FORMS, f32_routes=None, twin=False):
    """fp64: every form on the first route against the restatement, every other route (and, twin=True, the general-sort
    twin of a CSR route) bit-equal to it, a second build bit-equal; fp32: one full-form plan per route."""
    ref = t.ref()
    dev = _Dev(torch, t, F64)
    for form in forms:
        first = read(dev, t, routes[0], form, F64)
        B.check_readback(ref, dev.cells, B.Readback(first.nnz, first.den, first.probe))
        same_bits(read(dev, t, routes[0], form, F64), first, "%s: second build, %s" % (t.name, form))
        for route in routes[1:]:
            same_bits(read(dev, t, route, form, F64), first, "%s: %s against %s, %s" % (t.name, route, routes[0], form))
        if twin:
            for route in routes:
                if route != "coo":
                    same_bits(read(dev, t, route, form, F64, general_sort=True), first,
                              "%s: general sort of %s, %s" % (t.name, route, form))
    f32_routes = routes if f32_routes is None else f32_routes
    dev32 = _Dev(torch, t, F32) if f32_routes else None
    for route in f32_routes:
        got = read(dev32, t, route, "full", F32)
        B.check_readback(ref, dev32.cells, B.Readback(got.nnz, got.den, got.probe), F32)
    return ref


ALL_ROUTES = ("coo", "csr", "csr_sorted")


# ---- 1. row counts at the edges of rounds, wave slices, sort tiles and scan tiles ----------------------------------------------------
@gpu
@pytest.mark.parametrize("n", B.EDGE_N)
def test_1_row_counts_at_the_edges(torch_cuda, n):
    """n rows (a few of them dropped) as COO, as CSR and as CSR with sorted columns; n rows without a dropped one, where
    sorted columns take the one-pass route (asserted in build()); n VALID rows with 41 dropped on top -- the rank scan and
    coalesce_kernel run over n_valid, the sort over n.  G = 300, R = 37."""
    walk(torch_cuda, table("edge_table", n, "total"), ALL_ROUTES)
    t = table("edge_table", n, "clean")
    rowptr, col, _ = routes_of(t)["csr_sorted"][1]
    assert t.expect_one_pass(rowptr, col) == 1
    walk(torch_cuda, t, ("csr_sorted", "coo", "csr"), twin=True, f32_routes=("csr_sorted",))
    walk(torch_cuda, table("edge_table", n, "valid"), ("coo", "csr"), forms=("full", "entries"), f32_routes=())


# ---- 2. the histogram scan across its tile -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", (65536, 65537))
def test_2_histogram_scan_across_its_tile(torch_cuda, n):
    """8 sort tiles x 256 digits = 2048 histogram entries = one scan tile; 9 tiles = 2304: the carry between scan tiles."""
    walk(torch_cuda, table("hist_table", n), ("coo", "csr"), f32_routes=("coo",))


# ---- 3. scan_top_kernel's second trip -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_valid,n_drop", ((2097152, 0), (2097153, 5000)))
def test_3_scan_top_second_trip(torch_cuda, n_valid, n_drop):
    """n_valid = 2,097,152 rows are exactly 1024 tile sums of the rank scan (one trip of scan_top_kernel's loop), one more is
    1025 (the second trip, with the carry).  COO, 30 % repeated rows, the whole W through the probe in the full form."""
    t = table("top_table", n_valid, n_drop)
    assert -(-t.n_valid // B.SCAN_TILE) == (1024 if n_drop == 0 else 1025)
    walk(torch_cuda, t, ("coo",), forms=("full",), f32_routes=())


# ---- 4. pass-count edges of the key sort --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("G,R,passes", B.KEY_PASS_SHAPES)
def test_4_pass_count_edges_of_the_key_sort(torch_cuda, G, R, passes):
    """range() just below and exactly at 2^16 and 2^24; the smallest and the largest possible key present; dropped rows, whose
    sentinel must sort behind the largest real key"""
    assert B.passes_for(B.key_range(G, R)) == passes
    walk(torch_cuda, table("pass_table", G, R), ALL_ROUTES, f32_routes=("coo",))


# ---- 5. pass-count edges of the region sort -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("G,R,passes", B.REGION_PASS_SHAPES)
def test_5_pass_count_edges_of_the_region_sort(torch_cuda, G, R, passes):
    """passes_for(R) at 2^8 and 2^16; region 0 and R - 1 hold pairs.  R >= 65,535 has more than 64 region blocks: the
    general sort even for ordered CSR without a dropped row (asserted in build() and here)."""
    assert B.passes_for(R) == passes
    forms = ALL_FORMS if R < 1000 else ("full", "entries")
    walk(torch_cuda, table("pass_table", G, R), ALL_ROUTES, forms=forms, f32_routes=("coo",))
    clean = table("pass_table", G, R, 0)
    rowptr, col, _ = routes_of(clean)["csr_sorted"][1]
    assert clean.expect_one_pass(rowptr, col) == (1 if R < 1000 else 0) and B.geometry(G, R)[0] == (1 if R < 1000 else 96)
    walk(torch_cuda, clean, ("csr_sorted", "coo"), forms=("entries",), twin=True, f32_routes=())


# ---- 6. runs for heads_kernel / coalesce_kernel ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_drop", (300, 0))
def test_6_runs_at_block_edges(torch_cuda, n_drop):
    """Runs of 1 .. 20,000 rows that begin at the last and at the first thread of a 256-thread block, straddle a block edge and
    end at n_valid (dropped rows behind, n_drop = 300); COO with every run's rows spread over the sort's rounds, wave slices
    and tiles, CSR with shuffled columns, CSR with sorted columns (n_drop = 0: the one-pass route, with its twin)."""
    t = table("runs_table", n_drop)
    assert all(len(v) > 100 for v in t.meta["spread"].values())
    walk(torch_cuda, t, ALL_ROUTES, twin=n_drop == 0)


# ---- 7. the CSR row search ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("maker", ("row_search_table", "one_row_table", "single_cell_table", "one_entry_rows_table"))
def test_7_csr_row_search(torch_cuda, maker):
    """empty rows at the head and the tail, 700 empty rows across a 256-entry block edge, rows that fill blocks exactly, one
    row that holds the table, G = 1, one entry per row -- as CSR, bit-equal to the same rows as COO"""
    walk(torch_cuda, table(maker), ("csr", "csr_sorted", "coo"), twin=True, f32_routes=("csr",))


# ---- 8. the one-pass partition beyond one tile, and its bins ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R,variant,pairs", ((64, "full", (8192, 8192)), (64, "edges", (8128, 8193)), (200, "full", (25600, 25600)),
                                              (200, "runs", None)))
def test_8_one_pass_chunks_beyond_one_tile(torch_cuda, R, variant, pairs):
    """chunks of exactly one 8192-pair tile, 64 short of it and one over it; 25,600 pairs (three tiles and a part, run[]
    carried from tile to tile); with runs of neighbouring entries.  One-pass, bit-equal to the general-sort twin."""
    t = table("filled_table", R, variant)
    assert pairs is None or t.meta["chunk_pairs"] == pairs
    rowptr, col, _ = routes_of(t)["csr_sorted"][1]
    assert t.expect_one_pass(rowptr, col) == 1
    walk(torch_cuda, t, ("csr_sorted", "coo"), twin=True, f32_routes=("csr_sorted",))


@gpu
@pytest.mark.parametrize("R,one_pass", ((44032, 1), (44033, 0)))
def test_8_one_pass_bin_limit(torch_cuda, R, one_pass):
    """64 region blocks = 1024 bins, pairs in bin 0 and bin 1023: the one-pass route; 65 blocks: the general sort"""
    t = table("bins_table", R)
    rowptr, col, _ = routes_of(t)["csr_sorted"][1]
    assert t.expect_one_pass(rowptr, col) == one_pass and B.geometry(256, R)[0] * 16 == (1024 if one_pass else 1040)
    walk(torch_cuda, t, ("csr_sorted",), twin=True, f32_routes=("csr_sorted",) if one_pass else ())


# ---- 9. denominators ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R", (12, 13, 14, 15))
def test_9_denominators(torch_cuda, R):
    """regions of 0 .. 1000 pairs, R mod 4 = 0 .. 3 (den_kernel's last workgroup partly idle), weights of both signs over 12
    decades -- the fsum bound is not vacuous -- and one region whose two pairs cancel: den exactly 0, NaN / +-inf in that
    column only"""
    t = table("den_table", R)
    ref = walk(torch_cuda, t, ("coo", "csr"), f32_routes=("coo",))
    dev = _Dev(torch_cuda, t, F64)
    got = read(dev, t, "coo", "full", F64)
    assert got.den[2] == 0.0 and (got.den[np.arange(R) != 2][ref.n_r[np.arange(R) != 2] > 0] != 0).all()
    bad = ~np.isfinite(got.probe)
    assert bad[:, 2].all() and not bad[:, ref.n_r > 0][:, np.flatnonzero(ref.n_r > 0) != 2].any()


# ---- row permutations of a table without repeated pairs ---------------------------------------------------------------------------------
@gpu
def test_row_order_leaves_no_trace_without_repeated_pairs(torch_cuda):
    """20,000 distinct pairs and 150 dropped rows, reversed and shuffled: nothing of the input order survives the sort"""
    t = table("distinct_table")
    ref = t.ref()
    dev = _Dev(torch_cuda, t, F64)
    for form in ALL_FORMS:
        first = read(dev, t, "coo", form, F64)
        B.check_readback(ref, dev.cells, B.Readback(first.nnz, first.den, first.probe))
        for how in ("reversed", "shuffled"):
            same_bits(read(dev, B.permuted(t, how), "coo", form, F64), first, "%s, %s" % (how, form))


# ---- 10. refusals keep their text -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("first,others", ((300, (8190, 8195, 15000)), (8191, (8192, 9000)), (8192, (8193, 19999)), (0, (255, 256))))
def test_10_first_bad_row_is_reported(torch_cuda, first, others):
    from climate_toolbox_amd import _lib
    from climate_toolbox_amd.engine import DensePlan
    cell, code, w = B.bad_rows_table(first, others)
    with pytest.raises(_lib.WaggError, match=r"segment %d out of range" % first):
        DensePlan.from_segments(cell, code, w, 300, 37, dtype=F64)
    bad_code = np.isin(np.arange(len(code)), [first] + list(others)) & (code >= 37)
    o = np.argsort(cell, kind="stable")
    ok_cell = (cell >= 0) & (cell < 300)
    o = o[ok_cell[o]]                                            # as CSR only a column can be out of range
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(cell[ok_cell], minlength=300))]).astype(np.int64)
    at = int(np.flatnonzero(bad_code[o])[0])
    with pytest.raises(_lib.WaggError, match=r"segment %d out of range" % at):
        DensePlan.from_csr(rowptr, code[o], w[o], 300, 37, dtype=F64)


@gpu
def test_10_first_decreasing_rowptr_is_reported(torch_cuda):
    from climate_toolbox_amd import _lib
    from climate_toolbox_amd.engine import DensePlan
    t = table("edge_table", 2049, "clean")
    rowptr, col, val = (np.array(a) for a in t.csr())
    rowptr[[40, 170, 290]] = rowptr[[41, 171, 291]] + 1          # rows 40, 170 and 290 end before they begin
    with pytest.raises(_lib.WaggError, match="rowptr decreases at row 40"):
        DensePlan.from_csr(rowptr, col, val, t.G, t.R)


# ---- the randomised driver's builder cases ----------------------------------------------------------------------------------------------
FUZZ_BUILD_CASES, FUZZ_BUILD_SEED = 30, 2028


@gpu
def test_randomised_builder_cases(torch_cuda):
    """tests/fuzz_gpu.py's build_case (FUZZ_BUILD=1), 30 seeded cases: random row counts up to 40,000, shares of repeated,
    dropped and spread rows, COO / shuffled CSR / ordered CSR -- the checks of this module"""
    from tests.test_gpu_dense_forms_small import _fuzz_module
    fz = _fuzz_module()
    rng = np.random.default_rng(FUZZ_BUILD_SEED)
    failures, tags = [], []
    for i in range(FUZZ_BUILD_CASES):
        tag, fails = fz.build_case(i, rng)
        tags.append(tag)
        assert fails is not None, "every case is compared"
        if fails:
            failures.append(tag + " | " + "; ".join(fails))
    assert not failures, "\n".join(failures)
    n = {r: sum("[route %s]" % r in tag for tag in tags) for r in ("coo", "csr", "csr_sorted")}
    print("builder cases:", n)
    assert min(n.values()) >= 4, n
