"""The case table of tests/graph_replay.py, checked without a GPU: it covers exactly the calls docs/STREAM_CAPTURE.md lists as
capturable (and DESIGN.md points there), every case's restatement runs on its inputs, and every mutation changes every case's
expected result -- so a replay that silently reused an earlier step's results differs from the expectation at every step."""
import os
import re

import numpy as np
import pytest

from tests import graph_replay as GR
from tests.test_stream_order_host import _stream_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def audit_table():
    """{call: capturable?} from the table of docs/STREAM_CAPTURE.md (a row may name several calls)"""
    rows = {}
    for line in open(os.path.join(ROOT, "docs", "STREAM_CAPTURE.md"), encoding="utf-8"):
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) < 3 or cells[1] not in ("capturable", "not capturable"):
            continue
        for name in re.findall(r"`([A-Za-z0-9_.]+)`", cells[0]):
            assert name not in rows, name
            rows[name] = cells[1] == "capturable"
    return rows


def test_the_audit_lists_every_stream_entry_point_and_design_md_points_to_it():
    rows = audit_table()
    assert set(rows) == set(_stream_entry_points()), sorted(set(rows) ^ set(_stream_entry_points()))
    assert rows["SparsePlan.apply"] and rows["quantile_select"] and not rows["take_axis"] and not rows["any_less"] and not rows["DensePlan.saw_inf"]
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert "**Stream capture**" in design and "docs/STREAM_CAPTURE.md" in design


def test_cases_cover_the_capturable_calls_and_no_other():
    rows = audit_table()
    named = {c.name for c in GR.CASES}
    assert named == {n for n, ok in rows.items() if ok}, sorted(named ^ {n for n, ok in rows.items() if ok})
    assert len(set(GR.IDS)) == len(GR.IDS)
    # every row-list family at both widths, fp32 and fp64; the dense forms the audit names
    for fam in GR.RL_ENGINE.values():
        assert {(c.label.split()[0], dt) for c, dt in GR.PARAMS if c.name == fam} == {("n5", GR.F32), ("n5", GR.F64), ("n1029", GR.F32), ("n1029", GR.F64)}
        assert any("empty" in c.label or not GR.RL.FAMILIES[c.family].splits for c in GR.CASES if c.name == fam), fam
    labels = " ".join(c.label for c in GR.CASES if c.name == "DensePlan.apply")
    for form in ("full-split", "full-exact", "tiles", "entries"):
        assert form in labels, form


@pytest.mark.parametrize("case,dtype", GR.PARAMS, ids=GR.IDS)
def test_every_mutation_changes_the_expected_result(case, dtype):
    inp = case.build(dtype)
    want = [case.expect(inp, [np.array(f) for f in inp.fields])]
    labels = ["clean (captured)"]
    for label, fields in GR.case_steps(case, inp):
        assert all(f.shape == g.shape and f.dtype == g.dtype for f, g in zip(fields, inp.fields)), label
        want.append(case.expect(inp, fields))
        labels.append(label)
    assert labels[1:] == list(GR.MUTATIONS)
    for a, b, la, lb in zip(want, want[1:], labels, labels[1:]):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert a.shape == b.shape
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        assert not same.all(), "%s: the expected result of %r equals that of %r" % (case.id, lb, la)
    # the restatement agrees with itself under the case's own comparison (the tolerance arithmetic runs on these inputs)
    out_dtype = case.out_dtype or dtype
    for (label, fields), w in zip([("captured", [np.array(f) for f in inp.fields])] + GR.case_steps(case, inp), want):
        case.compare(inp, np.asarray(w).astype(out_dtype), w, fields, inp.skip if label == "inf" else None)
        if label == "inf" and inp.inf_at is not None:
            assert np.isinf(fields[0][inp.inf_at]) and np.isnan(fields[0][inp.nan_cell]) and np.isnan(fields[0][inp.nan_row]).all()


def test_row_list_cases_split_where_the_family_splits():
    """two parts for the six families that split (the two-period lists), one for spells, rolling windows and quantiles (with the
    empty third period) -- by tests/rowlist_layout.py's restatement of the library's rule on the library's own *_work_bytes"""
    from climate_toolbox_amd import _lib
    L = _lib.load()
    seen = set()
    for case, dtype in GR.PARAMS:
        if not hasattr(case, "family"):
            continue
        d = case.build(dtype).aux
        fam = GR.RL.FAMILIES[case.family]
        split = 1 if case.status == "own word" else GR.rl_split(L, case.family, d, case.variant)       # (own word: no workspace either)
        assert split == case.parts, (case.id, split)
        assert case.parts == 2 or not fam.splits or "empty" in case.label or "own" in case.label, case.id
        assert d.P == (3 if "empty" in case.label or not fam.splits else 2) and len(d.rows) == 37 and d.T == 40
        seen.add(case.family)
    assert seen == set(GR.RL_ENGINE)


def test_dense_cases_are_clean_up_to_capture_and_take_the_routes_their_labels_name():
    """The plain dense applies hold no NaN in the clean and the fresh field, so a fresh plan's warm-up leaves no non-finite note
    and the captured apply takes the route of a clean plan: the pack-free first pass (with the zero-fill of the gate word and the
    gated second pass) on the tile-sparse form at G = 384 and on the full exact / fp64 forms at T = 640 / 320 -- by
    tests/test_gpu_dense_forms_small.py's restatement of the rule -- and no other case.  k slices: the library's choice is 8
    everywhere (csrc/wagg_dense_route.cpp restated), one case hands in 16."""
    free = set()
    for case, dtype in GR.PARAMS:
        if not case.name.startswith("DensePlan."):
            continue
        inp = case.build(dtype)
        if case.name == "DensePlan.apply":
            assert np.isfinite(inp.fields[0]).all() and np.isfinite(case.fresh(inp)[0]).all(), case.id
        if case.pack_free[dtype]:
            free.add((case.label, np.dtype(dtype).name))
        assert case.k_slices[dtype] in (None, 1, 8, 16) and (case.k_slices[dtype] == 16) == ("ksplit 16" in case.label), case.id
    assert free == {("full-exact 384x689 T640", "float32"), ("full 384x689 T320", "float64"), ("tiles 384x689 T65", "float32"),
                    ("tiles 384x689 T65", "float64")}, free
