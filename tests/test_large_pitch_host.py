"""tests/large_pitch.py and the layouts of tests/test_gpu_large_pitch.py, without a GPU and without an allocation: conditions
on the INPUTS of the GPU cases, which must hold before any of them runs.

For every big buffer of every parametrised GPU case (LAYOUTS):
  * at least two rows start at or beyond LIMIT (a row AT 2^31 elements already has no signed 32-bit index) and at least one
    between LIMIT / 2 and LIMIT (where a sign-extended 32-bit offset turns negative);
  * every position a truncated row offset would read from (byte offset or element index cut to 32 bits, zero- or
    sign-extended) lies inside the buffer, and never inside the row it stands for -- so it holds sentinel or a foreign row;
  * the buffer is at most 40 GiB;
  * the rows are 16-byte aligned exactly when the case says so.
And once, for a segment-table case: the oracle on the field as each truncation would read it misses the true result by
orders of magnitude more than the case's tolerance."""
import numpy as np
import pytest

from tests import large_pitch as LP
from tests import test_gpu_fallback_routes as FR
from tests import test_gpu_large_pitch as GP

CASES = sorted(set(GP.LAYOUTS))


def test_every_gpu_case_is_listed():
    """(the parametrised lists of the GPU module and their layouts)"""
    ids = {c[0] for c in CASES}
    for i in GP.SEG_IDS:
        assert "a-" + i in ids
    for i in GP.DENSE_IDS:
        assert "e-" + i in ids
    for i in GP.RL_IDS:
        assert "f-" + i in ids
    assert {"b", "c-TR", "c-RT", "c-planes", "d", "f-out", "h-gather"} <= ids and len([i for i in ids if i.startswith("g-")]) == len(GP.PACK_CASES)
    tiers = {(c[3], c[4]) for c in CASES}
    assert tiers == {(4, "bytes"), (8, "bytes"), (4, "elems"), (8, "elems")}


@pytest.mark.parametrize("case,rows,cols,eb,tier,aligned,planes", CASES, ids=["%s-%dB" % (c[0], c[3]) for c in CASES])
def test_layout_conditions(case, rows, cols, eb, tier, aligned, planes):
    lead, pitch, total = LP.layout(rows, cols, eb, tier, aligned, planes)
    lim = LP.limit(eb, tier)
    n_rows = rows * planes
    starts = [r * pitch for r in range(n_rows)]
    assert sum(s >= lim for s in starts) >= 2, "two rows at or beyond LIMIT"
    assert sum(lim // 2 <= s < lim for s in starts) >= 1, "a row between LIMIT / 2 and LIMIT"
    assert total == lead + starts[-1] + cols and total * eb <= LP.MAX_BYTES
    assert lead % 4 == 0 and ((pitch * eb) % 16 == 0) == aligned and ((lead * eb) % 16 == 0)
    if aligned:
        assert pitch % 64 == 0
    wrapped = LP.wrapped_positions(n_rows, cols, lead, pitch, eb)
    assert len(wrapped) == n_rows and wrapped[0] == {}
    seen = set()
    for r, pos in enumerate(wrapped):
        true = lead + starts[r]
        for kind, p in pos.items():
            assert kind in LP.TRUNCATIONS
            assert 0 <= p and p + cols <= total, (r, kind, p)
            assert p + cols <= true or p >= true + cols, (r, kind, "reads the row it stands for")
            seen.add(kind)
    # the truncations the tier is about change at least two rows' addresses
    want = {"bytes-zext", "bytes-sext"} | ({"elems-sext"} if tier == "elems" else set())
    assert want <= seen
    for kind in want:
        assert sum(kind in pos for pos in wrapped) >= 2, kind


def test_layout_rejects_what_it_cannot_place():
    with pytest.raises(ValueError):
        LP.layout(3, 10, 4, "bytes")
    with pytest.raises(ValueError):
        LP.layout(6, 10, 4, "words")
    with pytest.raises(ValueError):
        LP.layout(1 << 20, 5000, 4, "bytes")


def test_wrapped_offsets_are_the_four_truncations():
    assert LP.wrapped_offsets(5, 4) == {}
    assert LP.wrapped_offsets(1 << 29, 4) == {"bytes-sext": -(1 << 29)}                      # 2^31 bytes
    assert LP.wrapped_offsets(1 << 30, 4) == {"bytes-zext": 0, "bytes-sext": 0}             # 2^32 bytes
    assert LP.wrapped_offsets(1 << 31, 4) == {"bytes-zext": 0, "bytes-sext": 0, "elems-sext": -(1 << 31)}
    assert LP.wrapped_offsets((1 << 32) + 7, 8) == {"bytes-zext": 7, "bytes-sext": 7, "elems-zext": 7, "elems-sext": 7}
    # the lead of LIMIT / 2 that would do for bytes does not for a signed element index: hence LIMIT in the "elems" tier
    lead, pitch, total = LP.layout(6, 1440, 4, "elems")
    assert lead == 1 << 31 and min(min(p.values(), default=0) for p in LP.wrapped_positions(6, 1440, lead, pitch, 4)) == 0


@pytest.mark.parametrize("tier", ["bytes", "elems"])
def test_a_truncated_offset_is_a_wrong_number_by_orders_of_magnitude(tier):
    """Segment-table case F-T6 (fp32, tier A and B): the oracle evaluated on the field as each truncation of the tier would
    read it -- rebuilt here from the case's small data and the sentinel -- against the true oracle.  The deviation (in units
    of max(|ref|, 1), the scale of the case's check) exceeds RTOL32 by more than a factor 100 for every truncation."""
    from oracle import ref_numpy as O
    from tests.test_gpu_parity import RTOL32
    T, dtype = 6, np.float32
    t = FR._table(*GP.SEG_GRID)
    X = FR._field(*GP.SEG_GRID, dtype, T)
    ref = FR._ref(*GP.SEG_GRID, dtype, T)
    lead, pitch, _ = LP.layout(T, t.G, 4, tier)
    kinds = ["bytes-zext", "bytes-sext"] + (["elems-sext"] if tier == "elems" else [])
    for kind in kinds:
        seen = LP.as_read_through(X, lead, pitch, 4, kind)
        changed = [r for r in range(T) if not np.array_equal(seen[r], X[r], equal_nan=True)]
        assert len(changed) >= 2, kind
        with np.errstate(invalid="ignore", over="ignore"):
            got = O.agg_coded(seen, t.cell, t.code, t.w, t.R)
        fin = np.isfinite(ref) & np.isfinite(got)
        with np.errstate(invalid="ignore"):
            rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
        dev = rel[fin]
        worst = float(dev.max())
        print("%s %s: rows %s read elsewhere, max deviation %.3g = %.3g x RTOL32" % (tier, kind, changed, worst, worst / RTOL32))
        assert worst > 100 * RTOL32, (kind, worst)
        # ... and in every row that was read elsewhere, not only in one
        for r in changed:
            assert rel[r][fin[r]].max() > 100 * RTOL32, (kind, r)
