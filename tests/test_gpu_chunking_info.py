"""wagg_plan_create over the tables of tests/chunk_dump.cpp (those with at least one row): every field of
wagg_plan_get_info and wagg_plan_get_den must be what tests/golden/plan_info.json records -- the values of the plan
builder BEFORE its host stages moved into csrc/wagg_chunk.cpp, recorded on an MI355X -- with the whole-line chunkings
built on threads, on the calling thread (WAGG_PLAN_SERIAL_BUILD) and not at all (WAGG_PLAN_NO_LINES)."""
import json
import os

import pytest

from climate_toolbox_amd import _lib
from tests.chunking_util import build_dump, dump_tables, plan_record

pytestmark = pytest.mark.gpu
FLAGS = {"default": 0, "no_lines": _lib.PLAN_NO_LINES, "serial": _lib.PLAN_SERIAL_BUILD}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    return dump_tables(build_dump(tmp_path_factory.mktemp("chunk_dump")))


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "plan_info.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def records(tables):
    L = _lib.load()
    return {t["name"]: {k: plan_record(L, t, f) for k, f in FLAGS.items()} for t in tables}


@pytest.mark.parametrize("flags", list(FLAGS))
def test_plan_info_and_den_as_recorded(records, golden, flags):
    assert set(records) == set(golden) and len(records) >= 24
    for name, want in golden.items():
        got = records[name][flags]
        assert set(got) == set(want[flags]), name
        for field, v in want[flags].items():
            assert got[field] == v, (name, flags, field)


def test_threaded_and_serial_builds_agree(records):
    for name, rec in records.items():
        assert rec["default"] == rec["serial"], name
        if rec["default"]["lines"]:
            assert rec["no_lines"]["lines"] == 0 and rec["no_lines"]["n_partial_rows"] == 0, name
