// Stand-alone dump of the host chunking stages (climate_toolbox_amd/csrc/wagg_chunk.h) for a built-in list of small
// tables: per table the coalesced table's den / nnz and, for the region-shaped, 32x8, 16x8 and 16x4 chunkings, the
// length and a 64-bit FNV-1a of every HostChunking array, the scalars and a few figures that show which branch of the
// builder a table took.  tests/test_chunking_host.py compares the output with tests/golden/chunkings.json.
//
//   chunk_dump            the dump, one JSON document (a table per line)
//   chunk_dump --tables   the tables themselves as JSON (tests/test_gpu_chunking_info.py builds plans from them)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../climate_toolbox_amd/csrc/wagg_chunk.h"

using namespace wagg;

struct Table {
    std::string name;
    int64_t G;
    int32_t R;
    int64_t row_len;
    std::vector<int32_t> cell, region;
    std::vector<double> w;
    void add(int64_t c, int32_t r, double wt) { cell.push_back((int32_t)c); region.push_back(r); w.push_back(wt); }
};

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static double weight_of(uint32_t &s) { return 0.25 + (double)(lcg(s) % 4096) / 1024.0; }   // exact in fp32 and fp64
static void shuffle(Table &t, uint32_t seed) {
    for (size_t i = t.cell.size(); i > 1; --i) {
        const size_t j = lcg(seed) % i;
        std::swap(t.cell[i - 1], t.cell[j]); std::swap(t.region[i - 1], t.region[j]); std::swap(t.w[i - 1], t.w[j]);
    }
}

static std::vector<Table> tables() {
    std::vector<Table> ts;
    uint32_t s = 12345;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // ---- degenerate tables
    ts.push_back({"empty", 64, 3, 16, {}, {}, {}});
    { Table t{"one_row", 64, 3, 16, {}, {}, {}}; t.add(37, 1, 2.5); ts.push_back(t); }
    { Table t{"all_null", 64, 3, 16, {}, {}, {}}; for (int i = 0; i < 5; ++i) t.add(7 * i, -1 - i, 1.0); ts.push_back(t); }
    { Table t{"all_nan", 64, 3, 16, {}, {}, {}}; for (int i = 0; i < 5; ++i) t.add(7 * i, i % 3, nan); ts.push_back(t); }
    { Table t{"no_regions", 64, 0, 16, {}, {}, {}}; for (int i = 0; i < 3; ++i) t.add(9 * i, -1, 1.0); ts.push_back(t); }
    // ---- sort paths: 16 x 32 grid, 8 regions in vertical stripes of 4 columns, every second cell in two regions
    auto stripes = [&](const char *name) {
        Table t{name, 512, 8, 32, {}, {}, {}};
        for (int64_t c = 0; c < 512; ++c) {
            const int32_t r = (int32_t)((c % 32) / 4);
            t.add(c, r, weight_of(s));
            if (c % 2) t.add(c, (r + 3) % 8, weight_of(s));
        }
        return t;
    };
    {
        Table t = stripes("rows_by_region_cell");
        std::vector<size_t> ix(t.cell.size());
        for (size_t i = 0; i < ix.size(); ++i) ix[i] = i;
        std::stable_sort(ix.begin(), ix.end(), [&](size_t a, size_t b) {
            return t.region[a] != t.region[b] ? t.region[a] < t.region[b] : t.cell[a] < t.cell[b]; });
        Table o{t.name, t.G, t.R, t.row_len, {}, {}, {}};
        for (size_t i : ix) o.add(t.cell[i], t.region[i], t.w[i]);
        ts.push_back(o);
    }
    ts.push_back(stripes("rows_by_cell"));
    {
        Table t = stripes("rows_shuffled_dups");
        for (int64_t c = 0; c < 512; c += 5) t.add(c, (int32_t)((c % 32) / 4), weight_of(s));   // duplicate (cell, region) pairs
        t.add(3, -1, 1.0); t.add(4, 2, nan);                                                   // a null label, a NaN weight
        shuffle(t, 99);
        ts.push_back(t);
    }
    {
        Table t{"wide_grid_stable_sort", (int64_t)1 << 23, 5, 4096, {}, {}, {}};                // G > 8 n + 2^22
        for (int i = 0; i < 100; ++i) t.add((int64_t)(lcg(s) % 2048) * 4096 + lcg(s) % 4096, (int32_t)(lcg(s) % 5), weight_of(s));
        t.add(t.cell[3], t.region[3], 1.5);
        ts.push_back(t);
    }
    // ---- region-shaped chunking (row_len = G: no whole-line chunkings)
    {
        Table t{"quads_64_and_65", 4096, 2, 4096, {}, {}, {}};
        for (int q = 0; q < 64; ++q) t.add(4 * q + q % 4, 0, weight_of(s));                    // exactly UQ quads: a normal group
        for (int q = 0; q < 65; ++q) t.add(1024 + 4 * q + q % 3, 1, weight_of(s));             // UQ + 1: giant
        ts.push_back(t);
    }
    for (int extra = 0; extra < 2; ++extra) {               // two regions over the same 64 quads = SEG_MAX segments; one more closes the group
        Table t{extra ? "group_513_segs" : "group_512_segs", 1024, 3, 1024, {}, {}, {}};
        for (int r = 0; r < 2; ++r) for (int c = 0; c < 256; ++c) t.add(c, r, weight_of(s));
        if (extra) t.add(255, 2, weight_of(s));
        ts.push_back(t);
    }
    for (int n = 127; n <= 128; ++n) {                      // RG_MAX one-cell regions share a group, one more opens the next
        Table t{n == 127 ? "group_127_regions" : "group_128_regions", 1024, n, 1024, {}, {}, {}};
        for (int r = 0; r < n; ++r) t.add(r, r, weight_of(s));
        ts.push_back(t);
    }
    {
        Table t{"giant_three_chunks", 4096, 1, 4096, {}, {}, {}};                              // 64 + 64 + 1 quads, 3 segments in the last
        for (int q = 0; q < 128; ++q) t.add(4 * q + 1, 0, weight_of(s));
        for (int k = 0; k < 3; ++k) t.add(4 * 128 + k, 0, weight_of(s));
        ts.push_back(t);
    }
    // ---- whole-line chunking
    auto blocks = [&](const char *name, int64_t n_rows, int64_t row_len, int64_t table_row_len) {   // compact regions of 7 x 9 cells, some ocean
        Table t{name, n_rows * row_len, (int32_t)(((n_rows + 6) / 7) * ((row_len + 8) / 9)), table_row_len, {}, {}, {}};
        for (int64_t r = 0; r < n_rows; ++r)
            for (int64_t c = 0; c < row_len; ++c) {
                if ((r * 31 + c * 17) % 11 == 0) continue;
                t.add(r * row_len + c, (int32_t)((r / 7) * ((row_len + 8) / 9) + c / 9), weight_of(s));
            }
        shuffle(t, 7);
        return t;
    };
    ts.push_back(blocks("lines_61x100", 61, 100, 100));                                         // row_len % 32 != 0
    ts.push_back(blocks("lines_row_len_20", 30, 20, 20));                                       // a strip shorter than a line
    ts.push_back(blocks("row_len_18_no_lines", 10, 18, 18));                                    // row_len % 4 != 0
    ts.push_back(blocks("row_len_G_no_lines", 61, 100, 6100));
    {
        Table t{"lines_closed_by_seg_max", 16 * 64, 3, 64, {}, {}, {}};                          // 96 segments a line: the 6th line is one too many
        for (int64_t c = 0; c < 16 * 64; ++c) for (int r = 0; r < 3; ++r) t.add(c, r, weight_of(s));
        ts.push_back(t);
    }
    {
        Table t{"lines_closed_by_rg_max", 8 * 32, 16 + 8 * 16, 32, {}, {}, {}};                  // 16 column regions + 16 new regions a line
        for (int64_t r = 0; r < 8; ++r)
            for (int64_t c = 0; c < 32; ++c) t.add(r * 32 + c, (int32_t)(c < 16 ? c : 16 + r * 16 + (c - 16)), weight_of(s));
        ts.push_back(t);
    }
    {
        Table t{"line_over_seg_max", 2 * 32, 17, 32, {}, {}, {}};                                // 32 cells x 17 regions = 544 segments in a line
        for (int64_t c = 0; c < 64; ++c) for (int r = 0; r < 17; ++r) t.add(c, r, weight_of(s));
        ts.push_back(t);
    }
    {
        Table t{"line_over_rg_max", 2 * 32, 128, 32, {}, {}, {}};                                // 32 cells x 4 regions of their own = 128 regions in a line
        for (int64_t c = 0; c < 32; ++c) for (int k = 0; k < 4; ++k) t.add(c, (int32_t)(4 * c + k), weight_of(s));
        t.add(40, 0, weight_of(s));
        ts.push_back(t);
    }
    {
        Table t{"scattered_partial_rows", 8320 * 32, 1, 32, {}, {}, {}};                         // 1040 chunks of one region: 1040 > 4 R + 1024
        for (int64_t r = 0; r < 8320; ++r) t.add(r * 32, 0, weight_of(s));
        ts.push_back(t);
    }
    {
        Table t{"quad0_unreferenced", 24 * 64, 4, 64, {}, {}, {}};                               // no row touches the first quad of any line
        for (int64_t r = 0; r < 24; ++r)
            for (int64_t c = 5; c < 64; c += 3) if (c % 32 >= 4) t.add(r * 64 + c, (int32_t)(r / 6), weight_of(s));
        ts.push_back(t);
    }
    return ts;
}

// ---- printing ---------------------------------------------------------------------------------------------------
template <typename T> static void arr(const char *name, const std::vector<T> &v, const char *sep = ", ") {
    uint64_t h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    printf("\"%s\": [%zu, \"%016llx\"]%s", name, v.size(), (unsigned long long)h, sep);
}
static void num(const char *name, long long v, const char *sep = ", ") { printf("\"%s\": %lld%s", name, v, sep); }

template <typename HC> static void print_chunking(const HC &c, bool lines) {
    printf("{");
    arr("grp_chunk_begin", c.grp_chunk_begin); arr("grp_giant", c.grp_giant);
    arr("chunk_u_begin", c.chunk_u_begin); arr("chunk_e_begin", c.chunk_e_begin);
    arr("ucell", c.ucell); arr("ent_region", c.ent_region); arr("ent_seg_begin", c.ent_seg_begin);
    arr("seg_u", c.seg_u); arr("seg_w", c.seg_w); arr("empty", c.empty); arr("chunk_desc", c.chunk_desc);
    arr("part_begin", c.part_begin); num("n_part_rows", c.n_part_rows);
    num("g0_normal", c.g0_normal); num("c0_normal", c.c0_normal); num("n_giant", c.n_giant);
    arr("ucell_c", c.ucell_c); arr("run_src", c.run_src); arr("run_len", c.run_len); num("Gc", c.Gc);
    arr("ucell_q", c.ucell_q); arr("run_src_q", c.run_src_q); arr("run_len_q", c.run_len_q); num("Gq", c.Gq);
    num("lines128", c.lines128); num("sectors64", c.sectors64);
    // figures derived from the arrays: which limits the chunks ran into
    const long long n_chunks = (long long)c.chunk_u_begin.size() - 1;
    long long quads_max = 0, segs_min = n_chunks ? (1ll << 40) : 0, segs_max = 0, ents_max = 0, quad0_unread = 0, quad0_unref = 0, unref = 0;
    for (long long k = 0; k < n_chunks; ++k) {
        const int32_t e0 = c.chunk_e_begin[(size_t)k], e1 = c.chunk_e_begin[(size_t)k + 1];
        const long long nseg = c.ent_seg_begin[(size_t)e1] - c.ent_seg_begin[(size_t)e0];
        quads_max = std::max<long long>(quads_max, c.chunk_u_begin[(size_t)k + 1] - c.chunk_u_begin[(size_t)k]);
        segs_min = std::min(segs_min, nseg); segs_max = std::max(segs_max, nseg);
        ents_max = std::max<long long>(ents_max, e1 - e0);
        bool read0 = false;
        for (int32_t q = c.ent_seg_begin[(size_t)e0]; q < c.ent_seg_begin[(size_t)e1]; ++q) read0 = read0 || ((c.seg_u[(size_t)q] & 0xff) >> 2) == 0;
        quad0_unread += !read0;
        if (lines) quad0_unref += c.ucell[(size_t)c.chunk_u_begin[(size_t)k]] & UCELL_UNREF;
    }
    if (lines) for (int32_t u : c.ucell) unref += u & UCELL_UNREF;
    num("n_chunks", n_chunks); num("n_groups", (long long)c.grp_giant.size());
    num("chunk_quads_max", quads_max); num("chunk_segs_min", segs_min); num("chunk_segs_max", segs_max); num("chunk_ents_max", ents_max);
    num("chunks_quad0_unread", quad0_unread); num("chunks_quad0_unref", quad0_unref); num("ucell_unref", unref, "");
    printf("}");
}

// which sort the kept rows of a table take in coalesce_table (its conditions, restated on the input)
static const char *sort_path(const Table &t) {
    bool by_cell = true, by_region_cell = true, first = true;
    int32_t pr = 0, pc = 0;
    long long kept = 0;
    for (size_t i = 0; i < t.cell.size(); ++i) {
        if (t.region[i] < 0 || std::isnan(t.w[i])) continue;
        if (!first) {
            by_cell = by_cell && pc <= t.cell[i];
            by_region_cell = by_region_cell && (pr < t.region[i] || (pr == t.region[i] && pc <= t.cell[i]));
        }
        first = false; pr = t.region[i]; pc = t.cell[i]; ++kept;
    }
    if (by_region_cell) return "none";
    if (t.G > 8 * kept + (1 << 22)) return "stable_sort";
    return by_cell ? "count_region" : "count_cell_region";
}

static void print_tables(const std::vector<Table> &ts) {
    printf("[\n");
    for (size_t k = 0; k < ts.size(); ++k) {
        const Table &t = ts[k];
        printf("{\"name\": \"%s\", \"G\": %lld, \"R\": %d, \"row_len\": %lld, \"cell\": [", t.name.c_str(), (long long)t.G, t.R, (long long)t.row_len);
        for (size_t i = 0; i < t.cell.size(); ++i) printf("%s%d", i ? "," : "", t.cell[i]);
        printf("], \"region\": [");
        for (size_t i = 0; i < t.region.size(); ++i) printf("%s%d", i ? "," : "", t.region[i]);
        printf("], \"w\": [");
        for (size_t i = 0; i < t.w.size(); ++i) { if (std::isnan(t.w[i])) printf("%sNaN", i ? "," : ""); else printf("%s%.17g", i ? "," : "", t.w[i]); }
        printf("]}%s\n", k + 1 < ts.size() ? "," : "");
    }
    printf("]\n");
}

static int dump_table(const Table &t) {
    SegTable st;
    ChunkError bad;
    if (!coalesce_table(t.cell.data(), t.region.data(), t.w.data(), (int64_t)t.cell.size(), t.G, t.R, t.row_len, st, bad)) {
        fprintf(stderr, "%s: %s\n", t.name.c_str(), bad.text.c_str());
        return 1;
    }
    printf("{\"name\": \"%s\", \"sort\": \"%s\", ", t.name.c_str(), sort_path(t));
    num("nnz", st.nnz); arr("den", st.den);
    const ChunkKnobs knobs;
    HostChunking c;
    chunk_regions(st, knobs, c);
    finish_chunking(c, false, false);
    printf("\"regions\": "); print_chunking(c, false);
    const int shapes[3][2] = {{32, 8}, {16, 8}, {16, 4}};
    for (const auto &sh : shapes) {
        printf(", \"%dx%d\": ", sh[0], sh[1]);
        if (!lines_applicable(st)) { printf("\"not applicable\""); continue; }
        if (!chunk_lines(st, sh[0], sh[1], knobs, c)) { printf("\"refused\""); continue; }
        finish_chunking(c, true, true);
        print_chunking(c, true);
    }
    printf("}");
    return 0;
}

int main(int argc, char **argv) {
    const std::vector<Table> ts = tables();
    if (argc > 1 && !strcmp(argv[1], "--tables")) { print_tables(ts); return 0; }
    printf("[\n");
    for (size_t k = 0; k < ts.size(); ++k) {
        if (dump_table(ts[k])) return 1;
        printf("%s\n", k + 1 < ts.size() ? "," : "");
    }
    printf("]\n");
    return 0;
}
