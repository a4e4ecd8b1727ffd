"""The schedule of a dense apply and the plan-time form choice (csrc/wagg_dense_route.h) on the CPU: tests/dense_route_dump.cpp,
linked against that unit alone, must print what tests/golden/dense_routes.json records -- the launch groups of every batch of
1 .. 4096 rows and of the batches around dense_rows_max line by line, the FNV-1a of the lines of 1 .. 200,000 rows, pick_ksplit,
the launch routes and the form of a table.  The golden values were recorded from the decision statements of dense_apply,
dense_apply_split, dense_build_image and pick_ksplit BEFORE they moved into the unit (copied into functions of the same
inputs, the self-recursion of dense_apply included, and linked with the same dump program): the row-group lines are the
proof that cutting a batch without the recursion launches the same groups.  (The file keeps the 2 x 4096 row-group lines
as runs of consecutive T with the same schedule -- a lossless packing of the recorder's output, checked against it when the
file was written; golden_group_lines unpacks it and every line is compared.)  The same program runs as a plain executable
under ASan + UBSan."""
import json
import os
import re
import subprocess

import pytest

from tests.chunking_util import ROOT, run_dump

MTS = {4: {1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 20, 21, 22, 23}, 8: {1, 2, 3, 4, 5, 6, 8, 10, 11}}


def build_dense_route_dump(outdir, target="dense_route_dump"):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "climate_toolbox_amd", "csrc"), target, "DENSE_ROUTE_OUT=" + str(outdir)])
    return os.path.join(str(outdir), target)


@pytest.fixture(scope="module")
def dump_text(tmp_path_factory):
    return run_dump(build_dense_route_dump(tmp_path_factory.mktemp("dense_route_dump")))


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "dense_routes.json")) as f:
        return json.load(f)


def golden_group_lines(golden, elem):
    """The recorded line of every T in 1 .. 4096.  The file holds them as runs [first T, last T, n_mb, MT, MT_tail] of equal
    schedules: MT_tail = 0 is one launch of n_mb blocks, otherwise n_mb full blocks and a launch of one block of MT_tail."""
    out = []
    for first, last, n_mb, MT, MT_tail in golden["groups_runs_e%d" % elem]:
        for T in range(first, last + 1):
            head = n_mb * MT * 16
            out.append("groups e%d T%d | 0+%d=%dx%d %d+%d=1x%d" % (elem, T, head, n_mb, MT, head, T - head, MT_tail) if MT_tail else
                       "groups e%d T%d | 0+%d=%dx%d" % (elem, T, T, n_mb, MT))
    assert [int(x.split()[2][1:]) for x in out] == list(range(1, 4097))
    return out


def test_same_schedule_as_before_the_move(dump_text, golden):
    lines = dump_text.splitlines()
    is_groups = lambda x: x.startswith("groups e")                                                 # noqa: E731
    want_groups = []
    for i, elem in enumerate((4, 8)):
        want_groups += golden_group_lines(golden, elem) + golden["groups_edges"][5 * i:5 * i + 5]
    got_groups = [x for x in lines if is_groups(x)]
    assert len(got_groups) == len(want_groups) == 2 * (4096 + 5)
    for got, want in zip(got_groups, want_groups):
        assert got == want
    rest = [x for x in lines if not is_groups(x)]
    assert len(rest) == len(golden["lines"])
    for got, want in zip(rest, golden["lines"]):
        assert got == want
    # the enumerations the issue of this unit asks for are all there
    for elem in (4, 8):
        assert any(x.startswith("groups_full e%d 200000 " % elem) for x in lines)
    assert any(x.startswith("ksplit_full 10240 ") for x in lines) and any(x.startswith("route_full ") for x in lines)


def test_clean_under_asan_ubsan(tmp_path_factory, dump_text):
    san = build_dense_route_dump(tmp_path_factory.mktemp("dense_route_dump_san"), "dense_route_dump_san")
    assert run_dump(san) == dump_text           # exit status 0 (run_dump), nothing preloaded, the same output


def _groups(dump_text):
    """{(elem, T): [(row0, rows, n_mb, MT), ...]}"""
    out = {}
    for line in dump_text.splitlines():
        m = re.match(r"groups e(\d) T(\d+) \|(.*)$", line)
        if m:
            out[int(m.group(1)), int(m.group(2))] = [tuple(int(v) for v in re.match(r"(\d+)\+(\d+)=(\d+)x(\d+)$", g).groups())
                                                     for g in m.group(3).split()]
    return out


def _routes(dump_text):
    out = []
    for line in dump_text.splitlines():
        if line.startswith("route e"):
            case, route = line.split(" | ")
            out.append((case.split()[1:], dict(kv.split("=") for kv in route.split())))
    return out


def test_hand_checked_row_groups(dump_text):
    g = _groups(dump_text)
    assert g[4, 365] == [(0, 365, 1, 23)]
    assert g[4, 1369] == [(0, 1056, 3, 22), (1056, 313, 1, 20)]
    assert g[4, 700] == [(0, 700, 2, 22)]                      # ragged, unsplit: the tail of 348 rows needs MT = 22 too
    assert g[4, 31] == [(0, 31, 1, 2)]
    assert g[8, 400] == [(0, 320, 2, 10), (320, 80, 1, 5)]
    assert g[8, 170] == [(0, 170, 1, 11)]
    # around dense_rows_max: 178 x 23 x 16 = 65,504 rows (fp32), 372 x 11 x 16 = 65,472 (fp64)
    assert g[4, 65504] == [(0, 65504, 178, 23)] and g[4, 65505] == [(0, 65504, 178, 23), (65504, 1, 1, 1)]
    assert g[8, 65472] == [(0, 65472, 372, 11)] and g[8, 65473] == [(0, 65472, 372, 11), (65472, 1, 1, 1)]
    assert g[4, 2 * 65504 + 1] == [(0, 65504, 178, 23), (65504, 65504, 178, 23), (131008, 1, 1, 1)]
    assert len(g[4, 547500]) == 10 and g[4, 547500][-2:] == [(524032, 23184, 63, 23), (547216, 284, 1, 18)]


def test_row_groups_tile_the_batch(dump_text):
    """Every printed batch: the groups follow one another without a gap, hold their rows, and use instantiated MTs only."""
    for (elem, T), gs in _groups(dump_text).items():
        at = 0
        for row0, rows, n_mb, MT in gs:
            assert row0 == at and rows > 0 and MT in MTS[elem], (elem, T, gs)
            assert (n_mb - 1) * MT * 16 < rows <= n_mb * MT * 16, (elem, T, gs)
            at += rows
        assert at == T, (elem, T, gs)


def test_every_case_takes_its_branch(dump_text):
    """Read from the dump itself, so that the reduced set cannot silently stop covering a branch of the schedule."""
    routes = _routes(dump_text)
    seen = lambda key: {r[key] for _, r in routes}                                                 # noqa: E731
    assert seen("form") == {"none", "split", "full", "tiled"}
    assert {r["img"] for _, r in routes if r["form"] == "split"} == {"0", "1"}
    assert seen("pf") == {"none", "tiled", "full"}
    assert all(r["form"] == "tiled" for _, r in routes if r["pf"] == "tiled")
    assert all(r["form"] == "full" and c[7] != "mb1" for c, r in routes if r["pf"] == "full")
    assert all(r["img"] == "0" for c, r in routes if c[7] != "mb1")
    assert len(seen("S")) >= 4                                  # the caller's ksplit and several of pick_ksplit's answers
    groups = _groups(dump_text)
    for elem in (4, 8):
        split = [gs for (e, T), gs in groups.items() if e == elem and T <= 4096 and len(gs) == 2]
        ragged_unsplit = [gs for (e, T), gs in groups.items() if e == elem and len(gs) == 1 and gs[0][2] >= 2 and T % (gs[0][3] * 16)]
        assert split and ragged_unsplit
        assert any(len(gs) > 2 for (e, T), gs in groups.items() if e == elem)                      # several dense_rows_max groups
        # every MT of the set is handed out at least once, and no other
        assert {g[3] for (e, T), gs in groups.items() if e == elem for g in gs} == MTS[elem]
    forms = [x for x in dump_text.splitlines() if x.startswith("form ")]
    assert {x.split(" | ")[1] for x in forms} == {"tiled=0 entries=0", "tiled=1 entries=0", "tiled=0 entries=1"}
