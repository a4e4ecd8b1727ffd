"""The route of a segment-table apply (csrc/wagg_route.h) on the CPU: tests/route_dump.cpp, linked against that unit alone,
must print what tests/golden/routes.json records -- the routes of the reduced set line by line and the FNV-1a of the full
product's lines.  The golden values were recorded from the decision statements of launch_sparse BEFORE they moved into the
unit (copied into a function of the same inputs and linked with the same dump program), so a route that changes shows here
even where the result on the GPU would stay right.  The same program runs as a plain executable under ASan + UBSan."""
import json
import os
import subprocess

import pytest

from tests.chunking_util import ROOT, run_dump


def build_route_dump(outdir, target="route_dump"):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "climate_toolbox_amd", "csrc"), target, "ROUTE_OUT=" + str(outdir)])
    return os.path.join(str(outdir), target)


@pytest.fixture(scope="module")
def dump_text(tmp_path_factory):
    return run_dump(build_route_dump(tmp_path_factory.mktemp("route_dump")))


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "routes.json")) as f:
        return json.load(f)


def test_same_routes_as_before_the_split(dump_text, golden):
    lines = dump_text.splitlines()
    assert lines[-1] == "full %d %s" % (golden["full_cases"], golden["full_fnv1a"])
    assert len(lines) - 1 == len(golden["reduced"])
    for got, want in zip(lines, golden["reduced"]):
        assert got == want


def test_clean_under_asan_ubsan(tmp_path_factory, dump_text):
    san = build_route_dump(tmp_path_factory.mktemp("route_dump_san"), "route_dump_san")
    assert run_dump(san) == dump_text           # exit status 0 (run_dump), nothing preloaded, the same output


def _cases(dump_text):
    out = []
    for line in dump_text.splitlines()[:-1]:
        case, route = line.split(" | ")
        out.append((case.split(), dict(kv.split("=") for kv in route.split())))
    return out


def test_every_case_takes_its_branch(dump_text):
    """Read from the dump itself, so that the reduced set cannot silently stop covering a branch of the route."""
    cases = _cases(dump_text)
    routes = [r for _, r in cases]
    seen = lambda key: {r[key] for r in routes}                                                    # noqa: E731
    assert seen("main") == {"none", "lcv", "lc_mfma", "stream"}
    assert seen("fin") == {"none", "fill", "transpose", "transpose+fill", "combine"}
    assert seen("refuse") == {"0", "1", "2"}
    assert seen("per_power") == {"0", "1"}
    assert seen("ch") == {"R", "L32", "L64", "L64e"}
    assert seen("gnthr") == {"1", "4"} and seen("gvec") == {"0", "1"}
    lcv = [r for r in routes if r["main"] == "lcv"]
    for key, want in (("vec", {"0", "1"}), ("edd", {"0", "1"}), ("gt", {"0", "1"}), ("planes", {"1", "2", "4"})):
        assert {r[key] for r in lcv} == want, key
    assert {r["vec"] for r in routes if r["main"] == "stream"} == {"0", "1"}
    # a main kernel beside the gather kernel's giant arm, the gather kernel alone, and nothing at all (no groups, T = 0)
    assert any(r["main"] != "none" and r["gather"] != "0" for r in routes)
    assert any(r["main"] == "none" and r["gather"] != "0" for r in routes)
    assert any(c[-2] == "T0" and r["main"] == "none" and r["gather"] == "0" and r["via_ws"] == "0" for c, r in cases)
    # the rows and brackets of the table on a plan with every chunking and no flag: (element, layout, transform) -> chunking
    table = {("e4", "TG", "none"): "L32", ("e8", "TG", "none"): "L64", ("e4", "GT", "none"): "R", ("e8", "GT", "none"): "L64",
             ("e4", "TG", "p1x4"): "L32", ("e8", "TG", "p1x4"): "L64", ("e4", "GT", "p1x4"): "R", ("e8", "GT", "p1x4"): "L64",
             ("e4", "TG", "edd4"): "L64", ("e8", "TG", "edd4"): "L64e", ("e4", "GT", "edd4"): "L64", ("e8", "GT", "edd4"): "L64e"}
    base = "f0 h7 {} TR {} c0 a1 g0 s1 ne0 cq1 T65 ldx64"
    found = {}
    for c, r in cases:
        key = (c[0], c[3], c[5])
        if key in table and " ".join(c[1:]) == base.format(c[3], c[5]):
            found[key] = (r["main"], r["ch"], r["planes"], r["per_power"])
    assert found == {k: ("lcv", ch, "4" if k[2] != "none" else "1", "0") for k, ch in table.items()}
    # the refusals occur with compact rows only, and one power per pass with fused powers only
    assert all(c[6] != "c0" for c, r in cases if r["refuse"] != "0")
    assert all(c[5] in ("p1x2", "p1x4", "p1x5") for c, r in cases if r["per_power"] == "1")
    assert any(c[5] == "p1x5" and r["per_power"] == "1" for c, r in cases)
