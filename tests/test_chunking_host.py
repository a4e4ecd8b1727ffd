"""Host chunking stages (csrc/wagg_chunk.h) on the CPU: tests/chunk_dump.cpp, linked against that unit alone, must print
for every built-in table what tests/golden/chunkings.json records -- the lengths, FNV-1a hashes and scalars of the arrays
the builder produced BEFORE the stages were split out of wagg_plan_create (dumped from that code where it uploaded them).
The same program runs as a plain executable under AddressSanitizer + UBSan, which is the only sanitizer run that reaches
the whole-line chunker (without a GPU wagg_plan_create skips it)."""
import json
import os

import pytest

from tests.chunking_util import SHAPES, build_dump, run_dump


@pytest.fixture(scope="module")
def dump_text(tmp_path_factory):
    return run_dump(build_dump(tmp_path_factory.mktemp("chunk_dump")))


@pytest.fixture(scope="module")
def dump(dump_text):
    return {t["name"]: t for t in json.loads(dump_text)}


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "chunkings.json")) as f:
        return {t["name"]: t for t in json.load(f)}


def test_same_arrays_as_before_the_split(dump, golden):
    assert list(dump) == list(golden)
    for name, want in golden.items():
        got = dump[name]
        assert set(got) == set(want), name
        for key, val in want.items():
            if isinstance(val, dict):
                assert isinstance(got[key], dict), (name, key, got[key])
                assert set(got[key]) == set(val), (name, key)
                for field, v in val.items():
                    assert got[key][field] == v, (name, key, field)
            else:
                assert got[key] == val, (name, key)


def test_clean_under_asan_ubsan(tmp_path_factory, dump_text):
    san = build_dump(tmp_path_factory.mktemp("chunk_dump_san"), "chunk_dump_san")
    assert run_dump(san) == dump_text           # exit status 0 (run_dump), nothing preloaded, the same output


def built(t, shape):
    assert isinstance(t[shape], dict), (t["name"], shape, t[shape])
    return t[shape]


def test_every_table_takes_its_branch(dump):
    """Read from the dump itself, so that a table cannot silently stop covering the branch it is there for."""
    na, refused = "not applicable", "refused"
    # degenerate tables: nothing kept, no chunk, no line chunkings
    for name in ("empty", "all_null", "all_nan", "no_regions"):
        t = dump[name]
        assert t["nnz"] == 0 and t["regions"]["n_chunks"] == 0 and t["regions"]["n_groups"] == 0
        assert all(t[s] == na for s in SHAPES)
    assert dump["no_regions"]["den"][0] == 0 and dump["empty"]["den"][0] == 3
    assert dump["one_row"]["nnz"] == 1 and all(built(dump["one_row"], s)["n_chunks"] == 1 for s in SHAPES)
    # sort paths, and the rows they leave: 768 distinct pairs however the 768 + duplicates arrive
    assert dump["rows_by_region_cell"]["sort"] == "none"
    assert dump["rows_by_cell"]["sort"] == "count_region"
    assert dump["rows_shuffled_dups"]["sort"] == "count_cell_region"
    assert dump["wide_grid_stable_sort"]["sort"] == "stable_sort" and dump["wide_grid_stable_sort"]["nnz"] <= 100
    for name in ("rows_by_cell", "rows_shuffled_dups"):
        assert dump[name]["nnz"] == dump["rows_by_region_cell"]["nnz"] == 768
        for s in ("regions",) + SHAPES:             # the same structure from every row order (the weights differ)
            for field in ("ucell", "seg_u", "ent_region", "chunk_desc"):
                assert dump[name][s][field] == dump["rows_by_region_cell"][s][field], (name, s, field)
    # region-shaped chunks: UQ = 64 quads, SEG_MAX = 512 segments, RG_MAX = 127 regions, NWAVE = 4
    r = dump["quads_64_and_65"]["regions"]
    assert (r["n_giant"], r["n_groups"], r["n_chunks"], r["chunk_quads_max"], r["g0_normal"]) == (1, 2, 3, 64, 1)
    r = dump["group_512_segs"]["regions"]
    assert (r["n_groups"], r["chunk_segs_max"], r["n_giant"]) == (1, 512, 0)
    r = dump["group_513_segs"]["regions"]
    assert (r["n_groups"], r["chunk_segs_max"], r["chunk_segs_min"], r["n_giant"]) == (2, 512, 1, 0)
    r = dump["group_127_regions"]["regions"]
    assert (r["n_groups"], r["chunk_ents_max"]) == (1, 127)
    r = dump["group_128_regions"]["regions"]
    assert (r["n_groups"], r["chunk_ents_max"], r["chunk_segs_min"]) == (2, 127, 1)
    r = dump["giant_three_chunks"]["regions"]
    assert (r["n_giant"], r["n_groups"], r["n_chunks"], r["chunk_segs_min"], r["c0_normal"]) == (1, 1, 3, 3, 3)
    # whole-line chunks
    for name in ("lines_61x100", "lines_row_len_20"):
        for s in SHAPES:
            c = built(dump[name], s)
            assert c["n_part_rows"] == c["ent_region"][0] > 0 and c["part_begin"][0] == dump[name]["den"][0] + 1
            assert c["ucell_unref"] > 0 and 0 < c["Gq"] <= c["Gc"] and c["chunks_quad0_unref"] == 0    # (quads behind the row end repeat)
    assert all(dump[n][s] == na for n in ("row_len_18_no_lines", "row_len_G_no_lines") for s in SHAPES)
    c = built(dump["lines_closed_by_seg_max"], "32x8")      # 5 + 5 + 5 + 1 lines a strip instead of 8 + 8
    assert (c["n_chunks"], c["chunk_segs_max"], c["chunk_quads_max"]) == (8, 480, 40)
    assert built(dump["lines_closed_by_seg_max"], "16x8")["chunk_quads_max"] == 32     # (eight lines: not closed early)
    c = built(dump["lines_closed_by_rg_max"], "32x8")       # 6 + 2 lines: a 7th would bring region 128
    assert (c["n_chunks"], c["chunk_ents_max"], c["chunk_quads_max"]) == (2, 112, 48)
    c = built(dump["lines_closed_by_rg_max"], "16x8")       # the strip of the per-line regions: 7 + 1 lines
    assert (c["n_chunks"], c["chunk_ents_max"]) == (3, 112)
    for name in ("line_over_seg_max", "line_over_rg_max"):
        assert dump[name]["32x8"] == refused and built(dump[name], "16x8") and built(dump[name], "16x4")
    assert all(dump["scattered_partial_rows"][s] == refused for s in SHAPES)
    for s in SHAPES:                                        # quad 0 of a chunk: read by no segment, yet not marked
        c = built(dump["quad0_unreferenced"], s)
        assert c["chunks_quad0_unread"] > 0 and c["chunks_quad0_unref"] == 0 and c["ucell_unref"] > 0 and c["Gq"] < c["Gc"]
