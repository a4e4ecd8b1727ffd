"""tests/rowlist_layout.py without a GPU: the case table against the row-list entry points the binding declares, the split the
GPU cases count on against the library's own *_work_bytes, and the layouts themselves -- where the poison stands, that every
route leaves a pad column, that the result window and its gaps are what tests/test_gpu_rowlist_layout.py says they are."""
import os
import re

import numpy as np
import pytest

from tests import rowlist_layout as RL

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wagg.h")


def test_the_case_table_names_every_row_list_entry_point():
    """A family is an export wagg_<name>_reduce_f32 -- or wagg_quantile_select_f32 -- with its _f64 sibling: each has a row, each
    row has both, and its *_work_bytes is an export too, but for the period quantiles, which have none (fam.work_bytes is None:
    no such export exists, and the family never splits).  A tenth family cannot arrive without a row."""
    from climate_toolbox_amd import _lib
    found = {}
    for e in _lib.EXPORTS:
        m = re.fullmatch(r"(wagg_\w+_(?:reduce|select))_(f32|f64)", e)
        if m:
            found.setdefault(m.group(1), set()).add(m.group(2))
    assert found and all(v == {"f32", "f64"} for v in found.values()), found
    by_entry = {fam.entry: fam for fam in RL.FAMILIES.values()}
    assert len(by_entry) == len(RL.FAMILIES) == 9
    assert sorted(found) == sorted(by_entry), "tests/rowlist_layout.py FAMILIES and the declared wagg_*_reduce_* / _select_* differ"
    for name, fam in RL.FAMILIES.items():
        assert fam.name == name and fam.variants, name
        assert fam.entry == ("wagg_quantile_select" if name == "quantile" else "wagg_%s_reduce" % name), name
        assert [RL.symbol(fam, d) for d in RL.DTYPES] == [fam.entry + "_f32", fam.entry + "_f64"]
        assert all(RL.symbol(fam, d) in _lib.EXPORTS and hasattr(_lib.load(), RL.symbol(fam, d)) for d in RL.DTYPES), name
        if fam.work_bytes is None:
            assert name == "quantile" and not fam.splits and fam.counting and fam.count_extra == 0
            assert not any(e.startswith("wagg_quantile") and e.endswith("_work_bytes") for e in _lib.EXPORTS)
        else:
            assert fam.work_bytes in _lib.EXPORTS, name
        assert len({v.id for v in fam.variants}) == len(fam.variants)
    assert [n for n, f in RL.FAMILIES.items() if f.work_bytes is None] == ["quantile"]
    # the quantiles: 8 planes with max_rows = the longest list, 16 planes (the most: two a lane in fp32) with the limit itself
    qv = {v.id: v for v in RL.FAMILIES["quantile"].variants}
    assert sorted(qv) == ["higher-q16", "linear-q8"] and qv["linear-q8"].planes == len(RL.Q8) == 8
    assert qv["higher-q16"].planes == len(RL.Q16) == _lib.QUANT_MAX == 16 and RL.QUANT_ROWS_MAX == _lib.QUANT_ROWS_MAX
    assert qv["linear-q8"].p == ("linear", RL.Q8, None) and qv["higher-q16"].p == ("higher", RL.Q16, 1024)
    for lists, longest in (("small", 9), ("split", 70), ("long", 512)):
        assert RL.longest_list(RL.LISTS[lists][1]) == longest
        mid, keep = RL.FAMILIES["quantile"].middle(qv["linear-q8"], {"longest": longest})
        assert mid[1:] == [8, _lib.QUANT_LINEAR, longest] and list(keep[0]) == RL.Q8
        mid, keep = RL.FAMILIES["quantile"].middle(qv["higher-q16"], {"longest": longest})
        assert mid[1:] == [16, _lib.QUANT_HIGHER, 1024] and list(keep[0]) == RL.Q16
    # two groups of the family's *_GROUP for the grouped summing / counting families, 3 powers and 2 thresholds for the others
    groups = {"edd_ladder": _lib.EDD_LADDER_GROUP, "bin_days": _lib.BIN_GROUP, "hinge": _lib.HINGE_GROUP, "exposure": _lib.EXPOSURE_GROUP}
    for name, g in groups.items():
        assert any(g < v.planes <= 2 * g for v in RL.FAMILIES[name].variants), name
    for name in ("period", "season"):
        assert {(v.id, v.planes) for v in RL.FAMILIES[name].variants} == {("poly", 3), ("edd", 2)}
    assert any(max(v.p[0]) > 8 for v in RL.FAMILIES["rolling"].variants) and any(max(v.p[0]) <= 8 for v in RL.FAMILIES["rolling"].variants)


def test_the_split_the_gpu_cases_count_on():
    """T = 70 entries in ONE period: n_rows / P / 8 caps the split at 8 on every route, so every family that splits asks for
    8 parts of 8 * planes * P * n bytes (wagg_period_reduce_work_bytes among them); the small lists (17 entries in 3 periods)
    never split; the spells and the rolling extremes ask for nothing; the period quantiles have no *_work_bytes to ask: their
    "full" workspace is three parts, non-zero, and no size makes them split."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    T, rb, rows = RL.SPLIT
    assert T == 70 and len(rows) == 70 and len(rb) == 2 and len(set(rows)) == 69 and 41 not in rows
    Ts, rbs, rowss = RL.SMALL
    assert Ts == 23 and list(np.diff(rbs)) == [9, 8, 0] and 4 not in rowss
    for n in RL.NS:
        for planes in (1, 2, 3, 9):
            assert L.wagg_period_reduce_work_bytes(n, 1, 70, planes) == 8 * RL.SPLIT_PARTS * planes * 1 * n
        for fam in RL.FAMILIES.values():
            for v in fam.variants:
                full = RL.full_work_bytes(L, fam, v, n, 1, 70)
                if fam.work_bytes is None:
                    assert full == 3 * RL.per_part(v.planes, 1, n) > 0 and RL.full_work_bytes(L, fam, v, n, 3, 17) == 3 * RL.per_part(v.planes, 3, n)
                    assert not fam.splits and [RL.work_bytes_of(k, full, v.planes, 1, n) > 0 for k in RL.WORKS] == [True, True, True, False]
                    continue
                assert full == (RL.SPLIT_PARTS * RL.per_part(v.planes, 1, n) if fam.splits else 0), (fam.name, v.id, n)
                assert getattr(L, fam.work_bytes)(n, 3, 17, RL.work_count(fam, v)) == 0
                if fam.splits:
                    want = {"full": 8, "three": 3, "one": 1, "none": 1}
                    for lanes in (1, 2, 4):
                        assert {k: RL.expected_split(k, full, v.planes, 1, n, 70, lanes) for k in RL.WORKS} == want
                    assert RL.work_bytes_of("one", full, v.planes, 1, n) // RL.per_part(v.planes, 1, n) == 1
                    assert RL.work_bytes_of("three", full, v.planes, 1, n) < full


def test_the_split_rule_restated_and_the_shape_on_which_the_route_decides_it():
    """rule_split against the library: *_work_bytes is the larger of the rule at one and at four cells per lane, times
    8 * planes * P * n.  n = 4097 with 512 entries in one period is the first n at which one cell per lane wants fewer parts
    (61) than 16-byte pieces (64, the cap) -- so which route a call took shows in how much of the workspace it wrote."""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    for n in (1, 5, 257, 1029, 4096, 4097, 70000, 300000):
        for P, n_rows in ((1, 70), (3, 17), (1, 512), (4, 512), (1, 15), (1, 16), (2, 5000)):
            parts = max(RL.rule_split(n, P, n_rows, 1), RL.rule_split(n, P, n_rows, 4))
            assert L.wagg_period_reduce_work_bytes(n, P, n_rows, 2) == (parts * RL.per_part(2, P, n) if parts > 1 else 0), (n, P, n_rows)
            assert RL.rule_split(n, P, n_rows, 1) <= RL.rule_split(n, P, n_rows, 2) <= RL.rule_split(n, P, n_rows, 4)
    T, rb, rows = RL.LONG
    assert len(rows) == 512 and set(rows) == set(range(T)) and list(rb) == [0, 512]
    n = RL.LONG_N
    assert [RL.rule_split(n, 1, 512, v) for v in (1, 2, 4)] == [61, 64, 64] == [RL.LONG_PARTS[False]] + [RL.LONG_PARTS[True]] * 2
    assert all(RL.rule_split(m, 1, 512, 1) == RL.rule_split(m, 1, 512, 4) for m in range(1, n, 64))      # no smaller n tells them apart
    for dtype in RL.DTYPES:
        assert RL.is_wide("1", dtype, n, True) and not RL.is_wide("3b", dtype, n, True)
        assert RL.expected_split("full", 64 * RL.per_part(9, 1, n), 9, 1, n, 512, 1) == 61
    assert [c[:3] for c in RL.LONG_CASES] == [("long", "1", n), ("long", "3b", n)]


def test_the_cases_are_paired_over_routes_sizes_and_bases():
    assert len(set(RL.CASES)) == len(RL.CASES) == len(RL.CASE_IDS) == len(set(RL.CASE_IDS))
    for lists in ("small", "split"):
        mine = [c for c in RL.CASES if c[0] == lists]
        assert {c[1] for c in mine} == set(RL.ROUTES), lists                       # every route on both list shapes
        assert {c[2] for c in mine} == set(RL.NS) and {c[3] for c in mine} == {True, False} and {c[4] for c in mine} == {0, 1}, lists
    for route in RL.ROUTES:
        mine = [c for c in RL.CASES if c[1] == route]
        assert {c[2] for c in mine} == set(RL.NS), route                           # every n on every route
        assert {c[3] for c in mine} == {True, False} and {c[4] for c in mine} == {0, 1}, route
    assert set(RL.works_for("split")) == set(RL.WORKS) and "full" in RL.works_for("small")
    for fam in RL.FAMILIES.values():
        assert all(RL.variants_for(fam, r) for r in ("1", "2", "3"))
        assert bool(RL.variants_for(fam, "3b")) == any(v.two_fields for v in fam.variants)
    assert {f.name for f in RL.FAMILIES.values() if RL.variants_for(f, "3b")} == {"period", "season", "edd_ladder", "exposure"}


@pytest.mark.parametrize("dtype", RL.DTYPES, ids=["f32", "f64"])
def test_routes_and_poison(dtype):
    """ldx % V and the base offsets are the three facts rowlist_geometry looks at; every route leaves a pad column; the poison
    stands in the guards, the pads, the unlisted rows and the out-of-season days, and nowhere else."""
    V = RL.vec(dtype)
    assert V == (4 if dtype == RL.F32 else 2)
    for n in RL.NS:
        for route in RL.ROUTES:
            ld = RL.ldx_for(route, n, dtype)
            assert n < ld <= n + V and ld % V == (1 if route == "2" else 0), (route, n)
        assert RL.is_wide("1", dtype, n, True) and not RL.is_wide("2", dtype, n, False) and not RL.is_wide("3", dtype, n, False)
        assert RL.is_wide("3b", dtype, n, False) and not RL.is_wide("3b", dtype, n, True)
    assert [RL.shifts_for(r) for r in RL.ROUTES] == [(0, 0), (0, 0), (1, 1), (0, 1)]
    for lists in ("small", "split"):
        for seasoned in (True, False):
            d = RL.make_data(lists, 257, dtype, seasoned)
            listed = np.zeros(d.T, dtype=bool)
            listed[d.rows] = True
            assert not listed.all() and not d.live[~listed].any()                  # a row no list names
            assert d.live[listed].all() != seasoned and d.live.any()
            assert np.isnan(d.X[0, 0]) and d.live[0, 0] and np.isnan(d.X[:, 6]).all() and d.live[0, 6]
            assert np.isfinite(d.X[d.live & ~np.isnan(d.X)]).all() and np.isfinite(d.H[d.live & ~np.isnan(d.H)]).all()
            for route in ("1", "3"):
                ld, shift = RL.ldx_for(route, d.n, dtype), RL.shifts_for(route)[0]
                flat, start = RL.poisoned(d.X, d.live, ld, shift)
                assert start == RL.GUARD + shift and len(flat) == start + d.T * ld + RL.GUARD and flat.dtype == dtype
                body = flat[start:start + d.T * ld].reshape(d.T, ld)
                bad = lambda a: ~np.isfinite(a) | (a == dtype(1e30))
                assert bad(flat[:start]).all() and bad(flat[start + d.T * ld:]).all() and bad(body[:, d.n:]).all()
                assert bad(body[:, :d.n][~d.live]).all()
                assert np.array_equal(body[:, :d.n][d.live], d.X[d.live], equal_nan=True)
                kinds = set(np.flatnonzero([np.isnan(body[:, d.n:]).any(), (body[:, d.n:] == np.inf).any(), (body[:, d.n:] == -np.inf).any(),
                                            (body[:, d.n:] == dtype(1e30)).any()]))
                assert kinds == {0, 1, 2, 3}                                       # the pad columns see all four poisons
                z, zs = RL.zero_padded(d.X, ld, shift)
                zb = z[zs:zs + d.T * ld].reshape(d.T, ld)
                assert zs == shift and (zb[:, d.n:] == 0).all() and np.array_equal(zb[:, :d.n], d.X, equal_nan=True)
    inf = RL.make_data("small", 5, dtype, True, inf_at=(1, 0))
    assert inf.X[1, 0] == np.inf and inf.live[1, 0] and np.isinf(inf.X).sum() == 1


def test_the_result_window():
    """ldo = n + 5, out_pstride = P * ldo + 7, GUARD elements on either side; the sentinel is a NaN no arithmetic produces"""
    for planes, P, n, off in ((9, 3, 1029, 1), (2, 1, 5, 0)):
        lay = RL.out_layout(planes, P, n, off)
        idx = RL.inside_index(lay)
        assert lay.ldo == n + 5 and lay.pstride == P * lay.ldo + 7 and lay.start == RL.GUARD + off
        assert idx.shape == (planes, P, n) and len(np.unique(idx)) == idx.size
        assert idx.min() == lay.start and idx.max() + RL.GUARD < lay.total
        assert idx[1, 0, 0] - idx[0, 0, 0] == lay.pstride and (P == 1 or idx[0, 1, 0] - idx[0, 0, 0] == lay.ldo)
    f = np.array([RL.SENTINEL[4]], dtype=np.uint32).view(np.float32)
    g = np.array([RL.SENTINEL[8]], dtype=np.uint64).view(np.float64)
    assert np.isnan(f).all() and np.isnan(g).all()
    assert RL.SENTINEL[4] != np.array([np.nan], dtype=np.float32).view(np.uint32)[0] and RL.SENTINEL[4] < 1 << 31
    assert RL.SENTINEL[8] != np.array([np.nan], dtype=np.float64).view(np.uint64)[0] and RL.SENTINEL[8] < 1 << 63


def test_the_header_asks_element_alignment_of_out_dev():
    """The GPU cases put out_dev one ELEMENT past a 16-byte boundary because include/wagg.h asks no more of it: between the
    period totals and the packed rows the only alignment it states is the workspace's (work_dev, 8 bytes, by the shared argument
    check).  Should the header come to ask more of out_dev, the case belongs at that boundary."""
    text = open(HEADER).read()
    a, b = text.index("---- period totals"), text.index("---- packed rows")
    section = text[a:b]
    assert all(RL.symbol(fam, RL.F32) in section for fam in RL.FAMILIES.values())
    for line in section.splitlines():
        if "out_dev" in line:
            assert "align" not in line.lower(), line
