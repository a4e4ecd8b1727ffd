"""The host-side helpers of tests/test_gpu_dense_forms_small.py, without a GPU: lists_of and probe_expected against the
oracle on an identity field, the list lengths, tile emptiness and geometry every table claims, and -- once -- what the
impulse probe sees that a 280 +- 15 field under the old tolerance does not."""
import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, _rel_ok
from tests import test_gpu_dense_forms_small as D

ALL_TABLES = D.SMALL_TABLES + [D.LONG]
IDS = ["%dx%d" % gr for gr in ALL_TABLES]
# (n_rb, rw, n_chunks) as the issue states them per table
GEOMETRY = {(127, 15): (1, 1, 1), (128, 16): (1, 1, 1), (129, 17): (1, 2, 2), (385, 688): (1, 43, 4), (384, 689): (2, 22, 3),
            (333, 257): (1, 17, 3), (4229, 48): (1, 3, 34)}


@pytest.mark.parametrize("G,R", ALL_TABLES, ids=IDS)
def test_helpers_against_the_oracle_on_an_identity_field(G, R):
    """O.agg_coded of the identity field is W / den itself: probe_expected must equal it (NaN and +-inf included), and the
    entries lists_of counts are its non-zeros, list by list."""
    from oracle import ref_numpy as O
    t = D.table(G, R)
    W, has, den, ratio = D.probe_expected(t.cell, t.code, t.w, G, R)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = O.agg_coded(np.eye(G), t.cell, t.code, t.w, R)
    _rel_ok(ratio, ref, 1e-14)
    assert np.array_equal(has, W != 0), "no pair of these tables cancels to 0"
    n_rb, rw, n_chunks = D.geometry(G, R)
    counts = D.lists_of(t.cell, t.code, t.w, G, R)
    assert counts.sum() == has.sum()
    nz = np.nan_to_num(ref, nan=0.0, posinf=1.0, neginf=1.0) != 0      # the oracle's own non-zeros (den == 0: +-inf at a pair)
    for rb in range(n_rb):
        for c in range(n_chunks):
            for wave in range(16):
                r0 = (rb * 16 + wave) * rw
                assert counts[rb, c, wave] == nz[128 * c:128 * (c + 1), r0:min(r0 + rw, R)].sum(), (rb, c, wave)


@pytest.mark.parametrize("G,R", ALL_TABLES, ids=IDS)
def test_tables_have_the_geometry_lists_and_tiles_they_claim(G, R):
    t = D.table(G, R)
    assert D.geometry(G, R) == GEOMETRY[(G, R)]
    n_rb, rw, n_chunks = D.geometry(G, R)
    counts = D.lists_of(t.cell, t.code, t.w, G, R)
    print("%d x %d: n_rb %d, rw %d, %d chunks, %d rows, list lengths %d .. %d" % (G, R, n_rb, rw, n_chunks, len(t.cell), counts.min(), counts.max()))
    # what the tables are made of
    W, has, den, _ = D.expected(G, R)
    assert (t.code == -1).sum() >= 2 and np.isnan(t.w).sum() >= 2 and (t.w < 0).sum() == 4
    assert len(t.cell) > has.sum() + (t.code == -1).sum() + np.isnan(t.w).sum(), "duplicate rows"
    assert den[t.r_sum0] == 0 and has[:, t.r_sum0].sum() == 2
    assert all(W[g, r] < 0 for g, r in t.neg_pairs)
    assert not has[D.GAP[0]:D.GAP[1]].any() and has[0, 0] and has[G - 1, R - 1]
    assert (np.abs(den[den != 0]) > 0.05).all()
    # a wave without a region, regions past R in the last wave that has one
    waves_used = -(-R // rw) - 16 * (n_rb - 1)
    if (G, R) in ((127, 15), (129, 17)):
        assert waves_used < 16 and (counts[-1, :, waves_used:] == 0).all() and counts[-1, :, waves_used - 1].sum() > 0
    if (G, R) == (129, 17):
        assert 16 * n_rb * rw == 32 > R and counts[0, 1].sum() > 0 and has[128].sum() >= 2      # one cell in the second chunk
    if (G, R) == (384, 689):
        assert n_chunks % 2 == 1
    if R > 32:
        assert counts.max() > 128, "the small tables with many regions per wave reach the long-list loop too"
    # the designed lists of the long table, each in its own chunk
    if (G, R) == D.LONG:
        for i, n in enumerate(D.LONG_LENGTHS):
            assert counts[0, 1 + i, D.LONG_WAVE] == n
        assert set(D.LONG_LENGTHS) <= set(counts.ravel().tolist())
        assert counts.max() == 384 and counts[0, 14:33, D.LONG_WAVE].min() >= 200
    # the tile-sparse form: empty (k tile, column tile) pairs in both element types
    for dtype in (D.F32, D.F64):
        bk = D.BK[dtype]
        tiles = D.tiles_of(t.cell, t.code, t.w, G, R, bk)
        n_kt, n_nt = -(-G // bk), -(-R // 256)
        assert 0 < len(tiles) < n_kt * n_nt
        assert not any(kt in range(D.GAP[0] // bk, D.GAP[1] // bk) for kt, _ in tiles)
        assert len(tiles) == len({(g // bk, r // 256) for g, r in zip(*np.nonzero(has))})
    assert (G % 32 == 0) == ((G, R) in ((128, 16), (384, 689))) and (G % 16 == 0) == (G % 32 == 0)


def test_amplitudes_are_signed_powers_of_two():
    a = D.amplitudes(4229)
    assert set(np.abs(a).tolist()) == {2.0 ** k for k in range(-3, 4)}
    assert (np.sign(a[::2]) == 1).all() and (np.sign(a[1::2]) == -1).all()


def test_pack_free_rule_of_the_shapes_used():
    """the shapes of the route-state test: which of them start with a pack-free pass"""
    assert D.pack_free(384, D.F32, "full", "exact", 640, True) and D.pack_free(384, D.F64, "full", "", 320, True)
    assert not D.pack_free(384, D.F32, "full", "exact", 369, True) and not D.pack_free(384, D.F64, "full", "", 177, True)
    assert D.pack_free(128, D.F64, "tiles", "", 65, True) and not D.pack_free(333, D.F32, "tiles", "", 65, True)
    assert not D.pack_free(384, D.F32, "tiles", "", 65, False) and not D.pack_free(384, D.F32, "full", "split", 640, True)
    assert not D.pack_free(384, D.F32, "entries", "", 640, True)


def test_forced_form_cases_cover_the_forms():
    """the 40 seeded cases of tests/fuzz_gpu.py's forms_case, from their tags alone (no GPU): every form at least 8 times"""
    fz = D._fuzz_module()
    rng = np.random.default_rng(D.FUZZ_FORMS_SEED)
    n = D.form_counts([fz.forms_case(i, rng, run=False)[0] for i in range(D.FUZZ_FORMS_CASES)])
    assert min(n.values()) >= 8, n


def test_the_probe_sees_one_dropped_pair_and_the_old_check_does_not():
    """Sensitivity, on the host: a stand-in for a correct fp32 kernel (W and den rounded to fp32, one fp32 division) passes
    the probe against the table's expected values and fails it against those of the table without ONE pair of its longest
    list; the aggregate of a 280 +- 15 field over the full table, checked the old way (RTOL32 |ref|) against the oracle of
    the table without that pair, passes."""
    from oracle import ref_numpy as O
    G, R = D.LONG
    t = D.table(G, R)
    W, has, den, _ = D.expected(G, R)
    a = D.amplitudes(G)
    with np.errstate(divide="ignore", invalid="ignore"):
        got = ((a[:, None] * W).astype(np.float32) / den.astype(np.float32)[None, :]).astype(np.float64)
    D.probe_check(got, a, W, has, den, D.F32)
    counts = D.lists_of(t.cell, t.code, t.w, G, R)
    rb, c, wave = np.unravel_index(np.argmax(counts), counts.shape)
    assert counts[rb, c, wave] == 384 and wave == D.LONG_WAVE
    g0, r0 = 128 * c + 64, 3 * wave + 1                          # a pair in the middle of that list
    assert has[g0, r0]
    rows = ~((t.cell == g0) & (t.code == r0))
    cell, code, w = t.cell[rows], t.code[rows], t.w[rows]
    assert D.lists_of(cell, code, w, G, R)[rb, c, wave] == 383
    W1, has1, den1, _ = D.probe_expected(cell, code, w, G, R)
    with pytest.raises(AssertionError):
        D.probe_check(got, a, W1, has1, den1, D.F32)
    with pytest.raises(AssertionError):
        D.probe_check(got, a, W1, has1, den1, D.F32, split=True)
    rng = np.random.default_rng(0)
    X = (280 + 15 * rng.standard_normal((16, G))).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        full, less = O.agg_coded(X, t.cell, t.code, t.w, R), O.agg_coded(X, cell, code, w, R)
    dev = np.abs(full[:, r0] - less[:, r0]).max()
    print("one pair of %d dropped from region %d: the 280 +- 15 aggregate moves by %.2e K, tolerance %.2e K" % (
        has[:, r0].sum(), r0, dev, RTOL32 * 280))
    assert dev > 0
    _rel_ok(full, less, RTOL32)
