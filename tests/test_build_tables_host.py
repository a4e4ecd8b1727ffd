"""tests/build_tables.py without a GPU: the restated geometry against hand-computed values, the constructors' promises, the
restatement against a Python loop and against the oracle, the order-sensitive patterns, and the evidence that the
comparison of tests/test_gpu_build_small.py fails on the defects a builder can have -- where a check in the style of
tests/test_gpu_round4.py (a 280 +- 15 field, RTOL32) does not."""
import functools

import numpy as np
import pytest

from tests import build_tables as B
from tests.test_gpu_parity import RTOL32, _rel_ok


@functools.lru_cache(maxsize=None)
def table(maker, *args):
    return getattr(B, maker)(*args)


# ---- geometry, keys, pass counts --------------------------------------------------------------------------------------------------
def test_geometry_and_pass_counts_by_hand():
    # (G, R): n_rb = ceil(R / 688), rw = ceil(R / (16 n_rb)), n_chunks = ceil(G / 128); range = n_rb n_chunks 16 128 rw
    assert B.geometry(128, 496) == (1, 31, 1) and B.key_range(128, 496) == 63488 < 2 ** 16
    assert B.geometry(128, 512) == (1, 32, 1) and B.key_range(128, 512) == 65536 == 2 ** 16
    assert B.geometry(32640, 512) == (1, 32, 255) and B.key_range(32640, 512) == 16711680 < 2 ** 24
    assert B.geometry(32768, 512) == (1, 32, 256) and B.key_range(32768, 512) == 2 ** 24
    # the shapes straddle the edges: 2 | 3 passes at 2^16, 3 | 4 at 2^24
    assert [B.passes_for(B.key_range(G, R)) for G, R, _ in B.KEY_PASS_SHAPES] == [2, 3, 3, 4] == [p for _, _, p in B.KEY_PASS_SHAPES]
    assert [B.passes_for(x) for x in (0, 1, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24)] == [1, 1, 1, 2, 2, 3, 3, 4]
    assert [B.passes_for(R) for _, R, _ in B.REGION_PASS_SHAPES] == [1, 2, 2, 2, 3, 3] == [p for _, _, p in B.REGION_PASS_SHAPES]
    # the sentinel's low 8 p bits lie behind every real key of these shapes
    for G, R, p in B.KEY_PASS_SHAPES:
        assert B.KEY_DROPPED & (2 ** (8 * p) - 1) > B.key_range(G, R) - 1 == B.key_of(G - 1, R - 1, G, R)
    # region blocks: 64 x 688 = 44,032 regions are 1024 bins of the one-pass partition, one more region is 65 blocks
    assert B.geometry(256, 44032) == (64, 43, 2) and B.geometry(256, 44033) == (65, 43, 2)
    assert B.chunk_bin(0, 44031, 256, 44032) == 1023 and B.chunk_bin(0, 42, 256, 44032) == 0
    assert [B.geometry(128, R)[0] for R in (65535, 65536, 65537)] == [96, 96, 96] and B.geometry(300, 257) == (1, 17, 3)
    assert B.geometry(256, 64) == (1, 4, 2) and B.geometry(256, 200) == (1, 13, 2)
    # a key by hand: G = 300, R = 37 -> rw = 3; (cell 130, region 7): wave 2, j 1, chunk 1, cell in chunk 2
    assert B.key_of(130, 7, 300, 37) == (((0 * 3 + 1) * 16 + 2) * 128 + 2) * 3 + 1


@pytest.mark.parametrize("G,R", [(1, 1), (300, 37), (128, 512), (32768, 512), (256, 44033), (128, 65537), (2048, 1100)])
def test_key_decode_round_trip(G, R):
    cells = np.unique(np.concatenate([[0, G - 1], np.arange(0, G, max(1, G // 37)), [min(G - 1, 127), min(G - 1, 128)]]))
    regions = np.unique(np.concatenate([[0, R - 1], np.arange(0, R, max(1, R // 41))]))
    c, r = (a.ravel() for a in np.meshgrid(cells, regions, indexing="ij"))
    k = B.key_of(c, r, G, R)
    assert len(np.unique(k)) == len(k) and k.min() >= 0 and k.max() < B.key_range(G, R)
    c2, r2 = B.decode(k, G, R)
    np.testing.assert_array_equal(c2, c)
    np.testing.assert_array_equal(r2, r)
    # key order = (region block, chunk, wave, cell in chunk, region in wave)
    n_rb, rw, n_chunks = B.geometry(G, R)
    o = np.lexsort((r % rw, c % 128, (r // rw) % 16, c // 128, r // (16 * rw)))
    np.testing.assert_array_equal(np.argsort(k), o)


# ---- the order-sensitive patterns ---------------------------------------------------------------------------------------------------
def test_transposition_shares_of_the_patterns():
    """the shares in tests/build_tables.py's docstring; every swap (i, i + 1) with i >= 1 is shown by a pattern in use"""
    shares = B.transposition_shares()
    assert {L: sorted(s[0]) for L, s in shares.items()} == {3: [1], 4: [1, 2], 5: [2, 3], 6: [3, 4]}
    assert {L: s[1] for L, s in shares.items()} == {3: 2, 4: 3, 5: 4, 6: 5}
    shown = set().union(*(s[0] for s in shares.values()))
    assert shown == set(range(1, 5)) and all(0 not in s[0] for s in shares.values())
    rng = np.random.default_rng(1)
    for L in B.PATTERNS:
        ws = B.run_weights(L, rng)
        assert B.seq_sum(ws) == ws[-1] and 1 <= ws[-1] <= B.SMALL_MAX        # the table-order sum is the last small integer
    # long runs remember: 4 of the 5 neighbour swaps of every block show, at the head of the run as at its end
    long = B.run_weights(20000, rng)
    assert B.seq_sum(long) == 512.0 * 3999 + 256 + long[-1] + long[-2]
    for part in (long[:200], long[:10000], long):
        shown = B.detectable_swaps(part) if len(part) == 200 else [i for i in range(5000, 5200) if _swap_shows(part, i)]
        assert len(shown) >= 156 and all(i % 5 != 3 for i in shown), len(shown)
    for L in (7, 255, 256, 257, 8192, 8193):
        ws = B.run_weights(L, rng)
        assert len(ws) == L and B.seq_sum(ws) == 512.0 * (L // 5 - 1) + 256 + ws[-1] + ws[-2]


def _swap_shows(ws, i):
    sw = np.array(ws)
    sw[i], sw[i + 1] = ws[i + 1], ws[i]
    return B.differs(float(np.add.accumulate(sw)[-1]), float(np.add.accumulate(ws)[-1]))


def test_add_at_adds_in_table_order():
    """the restatement's np.add.at against a plain Python loop, on order-sensitive runs scattered through the table: equal bits"""
    t = table("runs_table", 300)
    ref = t.ref()
    loop = B.reference_loop(*t.coo(), t.R)
    assert len(loop) == ref.nnz
    np.testing.assert_array_equal(ref.ws, np.array([loop[(c, r)] for c, r in zip(ref.pair_cell.tolist(), ref.pair_region.tolist())]))
    # and the order matters on this table: the same rows backwards give other sums
    back = B.reference(t.cell[::-1], t.code[::-1], t.w[::-1], t.G, t.R)
    assert (back.ws != ref.ws).sum() > 100


def test_reference_agrees_with_the_oracle():
    """identity field, fp64, a table with repeated pairs of ordinary weights: W / den of the restatement = O.agg_coded"""
    from oracle import ref_numpy as O
    rng = np.random.default_rng(5)
    G, R = 200, 23
    lengths = rng.integers(1, 4, 1500)
    pc, pr = B.draw_pairs(rng, 1500, np.arange(G), R, (11,), [(0, 0), (G - 1, R - 1)])
    t = B.assemble("plain", G, R, pc, pr, lengths, rng, 60, w=rng.uniform(0.1, 1.0, lengths.sum()))
    ref = t.ref()
    W, has = B.probe_matrices(ref, np.arange(G))
    assert has.sum() == ref.nnz == 1500 and ref.den[11] == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        got = O.agg_coded(np.eye(G), *t.coo(), R)
        _rel_ok(W / ref.den[None, :], got, 1e-13)


# ---- the constructors' promises -----------------------------------------------------------------------------------------------------
def _carries_everything(t, drops=True):
    assert (t.code < 0).any() == (np.isnan(t.w).any()) == drops
    ref = t.ref()
    assert (ref.n_r == 0).any()


@pytest.mark.parametrize("n", B.EDGE_N)
def test_edge_tables(n):
    total, valid, clean = (table("edge_table", n, k) for k in ("total", "valid", "clean"))
    assert total.n == n and valid.n_valid == n and valid.n == n + 41 and clean.n == clean.n_valid == n
    assert total.n_valid < n or n < 8
    for t in (total, valid, clean):
        assert t.G == 300 and t.R == 37 and t.ref().n_r[18] == 0
        rowptr, col, _ = t.csr(sort_columns=True)
        assert t.expect_one_pass(rowptr, col) == (t.n_valid == t.n)
    if n >= 255:
        assert clean.ref().nnz < n and min(B.pattern_shares(clean).values()) > 0          # rows drawn with repetition
    if n >= 1023:
        assert min(B.pattern_shares(clean).values()) >= 0.2
    for unit in (B.ROUND, B.WAVE_SLICE, B.SORT_TILE):
        if n >= 2 * unit - 1 and n >= 255:
            assert len(total.meta["spread"][unit]) > 0, unit


def test_scan_tables():
    for n in (65536, 65537):
        t = table("hist_table", n)
        assert t.n == n and -(-n // B.SORT_TILE) * 256 == (2048 if n == 65536 else 2304)
        _carries_everything(t)
        assert min(B.pattern_shares(t).values()) >= 0.2 and all(len(v) > 1000 for v in t.meta["spread"].values())


def test_pass_tables():
    for G, R, _ in B.KEY_PASS_SHAPES + B.REGION_PASS_SHAPES:
        t = table("pass_table", G, R)
        _carries_everything(t)
        k = t.sorted_keys()
        assert k[0] == 0 and k[-1] == B.key_of(G - 1, R - 1, G, R) and len(B.probe_cells(t)) <= min(G, 512 + 32)
        assert {0, G - 1} <= set(B.probe_cells(t).tolist()) and t.ref().n_r[0] > 0 and t.ref().n_r[R - 1] > 0
        assert min(B.pattern_shares(t).values()) >= 0.2
    for G, R, _ in B.KEY_PASS_SHAPES:
        assert table("pass_table", G, R).sorted_keys()[-1] == B.key_range(G, R) - 1


def test_runs_tables():
    for n_drop, order in ((300, "scattered"), (0, "scattered"), (0, "csr_sorted")):
        t = B.runs_table(n_drop, order)                          # (its placements are asserted by the constructor)
        assert t.n_valid % B.BLOCK == 255 and t.n == t.n_valid + n_drop
        if order == "scattered":
            long = np.flatnonzero(t.meta["lengths"] >= 255)
            assert all(np.isin(long, t.meta["spread"][u]).all() for u in (B.ROUND, B.WAVE_SLICE, B.SORT_TILE))
            assert all(len(v) > 100 for v in t.meta["spread"].values())
        assert min(B.pattern_shares(t).values()) >= 0.2
        rowptr, col, _ = t.csr(sort_columns=True)
        assert t.expect_one_pass(rowptr, col) == (n_drop == 0)
        rowptr, col, _ = t.csr()
        assert t.expect_one_pass(rowptr, col) == (order == "csr_sorted")


def test_row_search_tables():
    t = table("row_search_table")                                # (its placements are asserted by the constructor)
    assert t.G == 1505 and (t.code < 0).any() and np.isnan(t.w).any()
    one = table("one_row_table")
    assert one.G == 500 and one.R == 3000 and (one.cell == 250).all() and one.n == 4000
    assert table("single_cell_table").G == 1 and table("single_cell_table").n == 300
    each = table("one_entry_rows_table")
    assert each.G == 1025 and (np.bincount(each.cell) == 1).all()


def test_one_pass_tables():
    for R, variant, pairs in ((64, "full", (8192, 8192)), (64, "edges", (8128, 8193)), (200, "full", (25600, 25600))):
        t = table("filled_table", R, variant)
        assert t.meta["chunk_pairs"] == pairs and t.n == t.n_valid
        rowptr, col, _ = t.csr(sort_columns=True)
        np.testing.assert_array_equal(col, t.code)               # it is in (cell, region) order as it stands
        assert t.expect_one_pass(rowptr, col) == 1
    t = table("filled_table", 200, "runs")
    assert min(t.meta["chunk_pairs"]) > 3 * B.SORT_TILE and min(B.pattern_shares(t).values()) >= 0.2
    for R, one_pass in ((44032, 1), (44033, 0)):
        t = table("bins_table", R)
        rowptr, col, _ = t.csr(sort_columns=True)
        assert t.expect_one_pass(rowptr, col) == one_pass and t.expect_one_pass(rowptr, col, general_sort=True) == 0


def test_den_tables():
    for R in (12, 13, 14, 15):
        t = table("den_table", R)
        ref = t.ref()
        assert tuple(ref.n_r[:10]) == B.DEN_COUNTS and ref.den[2] == 0 and (t.code < 0).any() and np.isnan(t.w).any()
        aw = np.abs(t.w[t.keep])
        assert aw.max() / aw.min() > 1e11 and (t.w[t.keep] < 0).mean() > 0.4
        # the bound is not vacuous: far below the denominators it is applied to, yet above one rounding of them
        big = ref.n_r > 2
        assert (ref.den_tol[big] < 1e-9 * np.abs(ref.den[big])).all() and (ref.den_tol[big] > 2.0 ** -53 * np.abs(ref.den[big])).all()


def test_tables_without_repeated_pairs():
    t = table("distinct_table")
    assert t.ref().nnz == t.n_valid == 20000 and t.n == 20150
    for how in ("reversed", "shuffled"):
        p = B.permuted(t, how)
        assert not np.array_equal(p.cell, t.cell)
        np.testing.assert_array_equal(p.ref().ws, t.ref().ws)


def test_bad_rows_tables():
    cell, code, w = B.bad_rows_table(300, (8190, 8195, 15000))
    bad = np.flatnonzero((code >= 37) | (cell < 0) | (cell >= 300))
    np.testing.assert_array_equal(bad, [300, 8190, 8195, 15000])
    assert len({int(b) // B.BLOCK for b in bad}) == 4 and bad[1] // B.SORT_TILE != bad[2] // B.SORT_TILE


# ---- sensitivity: the comparison fails on every defect; the round-4 style check does not ---------------------------------------------
def round4_style(ref, other, G, R):
    """tests/test_gpu_round4.py's check of a plan that holds `other`'s weights against `ref`'s: a 280 +- 15 field of 70 rows,
    |got - ref| <= RTOL32 |ref|"""
    X = 280 + 15 * np.random.default_rng(G + R).standard_normal((70, G))
    Wa, Wb = B.probe_matrices(ref, np.arange(G))[0], B.probe_matrices(other, np.arange(G))[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        _rel_ok(X @ Wb / Wb.sum(0)[None, :], X @ Wa / Wa.sum(0)[None, :], RTOL32)


def straddling_run(t):
    """a run of 3 .. 6 rows that, in sorted order, lies on both sides of a 256-thread block edge"""
    k = t.sorted_keys()
    head = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    length = np.diff(np.concatenate([head, [len(k)]]))
    i = np.flatnonzero((length >= 3) & (length <= 6) & (head // B.BLOCK != (head + length - 1) // B.BLOCK))[0]
    c, r = B.decode(k[head[i]], t.G, t.R)
    run = int(np.flatnonzero((t.meta["pair_cell"] == c) & (t.meta["pair_region"] == r))[0])
    assert t.meta["lengths"][run] == length[i]
    return run


@pytest.mark.parametrize("maker,args", [("top_table", (2097153, 5000)), ("runs_table", (300,)), ("filled_table", (200, "runs"))],
                         ids=["case3", "case6", "case8"])
def test_the_comparison_fails_on_every_defect(maker, args):
    """The readback of a builder that is right about the UNMUTATED table is compared against the restatement of the table
    with one defect: a swap of two neighbouring rows of a run, the last row of a run across a block edge lost, a pair in the
    neighbouring region, a run split in two.  check_probe (and for the split check_counts: nnz + 1) fails every time; the
    round-4 style check passes the first three."""
    t = table(maker, *args)
    ref = t.ref()
    cells = B.probe_cells(t)
    rb = B.ideal_readback(ref, cells)
    B.check_readback(ref, cells, rb)                             # right about its own table
    run = straddling_run(t)
    for what in ("swap", "drop", "move", "split"):
        mutated = B.reference(*B.mutate(t, what, run), t.G, t.R)
        with pytest.raises(AssertionError, match="weights wrong|must be 0"):
            B.check_probe(mutated, cells, rb)
        with pytest.raises(AssertionError):
            B.check_readback(mutated, cells, rb)
        if what == "split":
            assert mutated.nnz == ref.nnz + 1
            with pytest.raises(AssertionError, match="nnz"):
                B.check_counts(mutated, rb)
        else:
            assert mutated.nnz == ref.nnz or (what == "move" and mutated.nnz == ref.nnz - 1)     # (it may meet a pair there)
            round4_style(mutated, ref, t.G, t.R)                 # ... and this is what the suite had: it passes
    rb32 = B.ideal_readback(ref, cells, np.float32)
    B.check_readback(ref, cells, rb32, np.float32)
    with pytest.raises(AssertionError):
        B.check_probe(B.reference(*B.mutate(t, "swap", run), t.G, t.R), cells, rb32, np.float32)
