// Host chunking of a segment table (wagg_chunk.h): coalesce the rows, form whole-line or region-shaped chunks, finish
// them into the arrays the kernels read.  No HIP here -- wagg_sparse.hip uploads the result.
#include "wagg_chunk.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>

#include "../../include/wagg.h"

namespace wagg {

bool row_in_range(int64_t i, int32_t region, int32_t cell, int64_t G, int32_t R, ChunkError &err) {
    char text[128];
    if (!(region < R))
        snprintf(text, sizeof text, "region_code[%lld]=%d out of range [0,%d)", (long long)i, region, R);
    else if (!(cell >= 0 && cell < G))
        snprintf(text, sizeof text, "cell_idx[%lld]=%d out of range", (long long)i, cell);
    else return true;
    err.code = WAGG_EINVAL;
    err.text = text;
    return false;
}

bool coalesce_table(const int32_t *cell_idx, const int32_t *region_code, const double *w_eff, int64_t nseg, int64_t G, int32_t R,
                    int64_t row_len, SegTable &t, ChunkError &err) {
    t.G = G; t.R = R; t.row_len = row_len;
    std::vector<Seg> &segs = t.segs;
    t.den.assign((size_t)R, 0.0);
    segs.clear();
    segs.reserve((size_t)nseg);
    for (int64_t i = 0; i < nseg; ++i) {
        const int32_t r = region_code[i];
        if (r < 0) continue;                                  // null label (S3)
        if (!row_in_range(i, r, cell_idx[i], G, R, err)) return false;
        if (std::isnan(w_eff[i])) continue;                   // skipna on :78/:79
        t.den[(size_t)r] += w_eff[i];                         // aggregations.py:79
        segs.push_back({r, cell_idx[i], w_eff[i]});
    }
    // by (region, cell), rows of one pair in table order (S5: they are added in that order below).  std::stable_sort on
    // the 16-byte rows was half of a c2-real plan build (42 of ~80 ms for 4e5 rows); stable counting passes -- by cell,
    // then by region -- do it in a third of that, and a table that already comes by cell (rows = grid order, the usual
    // export) or by (region, cell) skips the passes it does not need
    {
        bool by_cell = true, by_region_cell = true;
        for (size_t i = 1; i < segs.size(); ++i) {
            by_cell = by_cell && segs[i - 1].cell <= segs[i].cell;
            by_region_cell = by_region_cell && (segs[i - 1].region < segs[i].region ||
                                                (segs[i - 1].region == segs[i].region && segs[i - 1].cell <= segs[i].cell));
        }
        auto counting_pass = [&](int64_t n_keys, auto key_of) {
            std::vector<int64_t> first((size_t)n_keys + 1, 0);
            for (const Seg &sg : segs) ++first[(size_t)key_of(sg) + 1];
            for (int64_t k = 0; k < n_keys; ++k) first[(size_t)k + 1] += first[(size_t)k];
            std::vector<Seg> sorted(segs.size());
            for (const Seg &sg : segs) sorted[(size_t)first[(size_t)key_of(sg)]++] = sg;
            segs.swap(sorted);
        };
        if (by_region_cell) {
            // nothing to do
        } else if (G > 8 * (int64_t)segs.size() + (1 << 22)) {          // a counter per cell would dwarf the table
            std::stable_sort(segs.begin(), segs.end(), [](const Seg &a, const Seg &b) {
                return a.region != b.region ? a.region < b.region : a.cell < b.cell;
            });
        } else {
            if (!by_cell) counting_pass(G, [](const Seg &sg) { return (int64_t)sg.cell; });
            counting_pass(R, [](const Seg &sg) { return (int64_t)sg.region; });
        }
    }
    // coalesce duplicate (cell, region) rows (S5)
    size_t m = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        if (m && segs[m - 1].region == segs[i].region && segs[m - 1].cell == segs[i].cell)
            segs[m - 1].w += segs[i].w;
        else segs[m++] = segs[i];
    }
    segs.resize(m);
    t.nnz = (int64_t)m;

    // per-region ranges
    t.rbeg.assign((size_t)R + 1, 0);
    for (const Seg &s : segs) t.rbeg[(size_t)s.region + 1]++;
    for (int32_t r = 0; r < R; ++r) t.rbeg[(size_t)r + 1] += t.rbeg[(size_t)r];
    return true;
}

// ---- whole-line plan (round 3) --------------------------------------------------------------------------------
// A chunk = up to 8 whole 32-cell LINES (128 bytes of a fp32 row, 256 of a fp64 row) of ONE column strip: the
// land lines of the strip in row order, eight at a time (ocean rows in between are skipped).  Every line belongs
// to exactly one chunk and is fetched whole: 8 line requests per timestep and chunk where the region-shaped
// chunks below need ~23 (their quads straddle lines, and border lines are fetched by both neighbours), at
// ~1.4x the bytes (the ocean cells of a coastal line come along).  The price: a region cut by a strip or by a
// group of eight lines becomes several (chunk, region) ENTRIES, each a partial sum with a row of its own in the
// partial buffer; combine_parts_kernel adds them up (1.6 rows per region on the 0.25-degree impact regions).
// Taken when the grid's row length is known (whole rows of whole quads) and the table is compact enough.
bool chunk_lines(const SegTable &t, int line_cells, int lines_per_chunk, const ChunkKnobs &knobs, HostChunking &c) {
    const std::vector<Seg> &segs = t.segs;
    const int64_t nnz = t.nnz, G = t.G, row_len = t.row_len;
    const int32_t R = t.R;
    const int LINE = line_cells;                                       // cells per line
    const int LPC = lines_per_chunk;                                   // lines per chunk
    c = HostChunking();
    c.seg_u.reserve((size_t)nnz); c.seg_w.reserve((size_t)nnz);

    struct LSeg { int64_t line; int32_t region, col; double w; };
    // segments by (line, region, column), line = strip * n_rows + row: `segs` is sorted by (region, cell), so a STABLE
    // counting sort on the line alone gives that order (cells of one line and region ascend with their column)
    const int64_t n_rows = G / row_len, n_strips = (row_len + LINE - 1) / LINE;
    std::vector<LSeg> ls((size_t)nnz);
    {
        std::vector<int64_t> first((size_t)(n_rows * n_strips) + 1, 0);
        std::vector<int64_t> line_of((size_t)nnz);
        for (int64_t i = 0; i < nnz; ++i) {
            const int64_t row = segs[(size_t)i].cell / row_len, col = segs[(size_t)i].cell % row_len;
            line_of[(size_t)i] = (col / LINE) * n_rows + row;
            ++first[(size_t)line_of[(size_t)i] + 1];
        }
        for (size_t l = 1; l < first.size(); ++l) first[l] += first[l - 1];
        for (int64_t i = 0; i < nnz; ++i) {
            const int64_t col = segs[(size_t)i].cell % row_len;
            ls[(size_t)first[(size_t)line_of[(size_t)i]]++] = {line_of[(size_t)i], segs[(size_t)i].region, (int32_t)(col % LINE), segs[(size_t)i].w};
        }
    }
    std::vector<std::vector<int32_t>> parts((size_t)R);
    std::vector<int32_t> region_mark((size_t)R, -1);
    struct CSeg { int32_t region, ulocal; double w; };
    // pass 1: form the chunks strip by strip
    struct LChunk { int64_t key; std::vector<int32_t> quads; std::vector<CSeg> cs; };
    std::vector<LChunk> chunks;
    size_t i = 0;
    while (i < ls.size()) {
        // one chunk: lines of this strip while it holds < LPC lines, <= SEG_MAX segments, <= RG_MAX regions
        const int64_t strip = ls[i].line / n_rows;
        const int32_t chunk_id = (int32_t)chunks.size();
        int n_lines = 0, n_regions = 0;
        LChunk ch;
        ch.key = ((ls[i].line % n_rows) / LPC) * n_strips + strip;       // band of LPC grid rows, then strip
        while (i < ls.size() && ls[i].line / n_rows == strip && n_lines < LPC) {
            size_t j = i;                                          // the segments of the next line
            int fresh = 0;
            while (j < ls.size() && ls[j].line == ls[i].line) {
                if (region_mark[(size_t)ls[j].region] != chunk_id) { region_mark[(size_t)ls[j].region] = chunk_id; ++fresh; }
                ++j;
            }
            if (n_lines > 0 && ((int64_t)ch.cs.size() + (int64_t)(j - i) > SEG_MAX || n_regions + fresh > RG_MAX)) {
                for (size_t k = i; k < j; ++k) region_mark[(size_t)ls[k].region] = -1;   // (marks of the line not taken)
                for (const CSeg &s : ch.cs) region_mark[(size_t)s.region] = chunk_id;
                break;
            }
            if ((int64_t)(j - i) > SEG_MAX || fresh > RG_MAX) return false;   // one line alone is too much
            n_regions += fresh;
            const int64_t row = ls[i].line % n_rows;
            for (int q = 0; q < LINE / 4; ++q) {                   // the line's quads; those behind the row end repeat its last
                int64_t c0 = strip * LINE + 4 * q;
                if (c0 + 4 > row_len) c0 = row_len - 4;
                ch.quads.push_back((int32_t)(row * row_len + c0));
            }
            for (size_t k = i; k < j; ++k) ch.cs.push_back({ls[k].region, n_lines * LINE + ls[k].col, ls[k].w});
            ++n_lines;
            i = j;
        }
        std::sort(ch.cs.begin(), ch.cs.end(), [](const CSeg &a, const CSeg &b) {
            return a.region != b.region ? a.region < b.region : a.ulocal < b.ulocal; });
        chunks.push_back(std::move(ch));
    }
    // pass 2: flatten, in the order formed (strip-major: down one column strip, then the next).  Measured against
    // band-major order (all strips of eight grid rows, then the next eight rows: neighbouring lines of the same
    // DRAM pages in flight together) on c2-real / c3-real: 0.236 / 0.331 ms strip-major, 0.237 / 0.352 ms
    // band-major (gpurun r3r) -- the diagnostic build keeps the switch
    if (knobs.lines_order == 2)
        std::stable_sort(chunks.begin(), chunks.end(), [](const LChunk &a, const LChunk &b) { return a.key < b.key; });
    int64_t n_part = 0;
    for (const LChunk &ch : chunks) {
        c.ucell.insert(c.ucell.end(), ch.quads.begin(), ch.quads.end());
        c.chunk_u_begin.push_back((int32_t)c.ucell.size());
        const std::vector<CSeg> &cs = ch.cs;
        // the chunk's entries, longest first: the consumer waves of sparse_lcv_kernel take them from a shared
        // counter, so the long ones start early and the short ones fill the end (longest-processing-time order)
        std::vector<std::pair<size_t, size_t>> runs;
        for (size_t k = 0; k < cs.size();) {
            size_t m2 = k;
            while (m2 < cs.size() && cs[m2].region == cs[k].region) ++m2;
            runs.push_back({k, m2});
            k = m2;
        }
        std::stable_sort(runs.begin(), runs.end(), [](const std::pair<size_t, size_t> &a, const std::pair<size_t, size_t> &b) {
            return a.second - a.first > b.second - b.first; });
        for (const auto &run : runs) {
            for (size_t m2 = run.first; m2 < run.second; ++m2) { c.seg_u.push_back(cs[m2].ulocal); c.seg_w.push_back(cs[m2].w); }
            parts[(size_t)cs[run.first].region].push_back((int32_t)n_part);
            c.ent_region.push_back((int32_t)n_part++);              // the entry's row in the partial buffer
            c.ent_seg_begin.push_back((int32_t)c.seg_u.size());
        }
        c.chunk_e_begin.push_back((int32_t)c.ent_region.size());
        c.grp_giant.push_back(0);
        c.grp_chunk_begin.push_back((int32_t)(c.chunk_u_begin.size() - 1));
    }
    // scattered regions (a c5-like table) would need more partial rows than the table has regions many times
    // over: such tables keep the region-shaped chunks (and usually take a dense-family form anyway)
    if (n_part > 4 * (int64_t)R + 1024) return false;
    // partial rows are numbered region-major: region r owns rows part_begin[r] .. part_begin[r + 1] - 1 of the
    // partial buffer, in chunk order, so the combine kernel streams the buffer front to back
    c.part_begin.assign((size_t)R + 1, 0);
    std::vector<int32_t> new_id((size_t)n_part, 0);
    for (int32_t r = 0; r < R; ++r) {
        c.part_begin[(size_t)r + 1] = c.part_begin[(size_t)r] + (int32_t)parts[(size_t)r].size();
        for (size_t j = 0; j < parts[(size_t)r].size(); ++j)
            new_id[(size_t)parts[(size_t)r][j]] = c.part_begin[(size_t)r] + (int32_t)j;
        if (parts[(size_t)r].empty()) c.empty.push_back(r);
    }
    for (int32_t &e : c.ent_region) e = new_id[(size_t)e];
    c.n_part_rows = n_part;
    return true;
}

void chunk_regions(const SegTable &t, const ChunkKnobs &knobs, HostChunking &c) {
    const std::vector<Seg> &segs = t.segs;
    const std::vector<int64_t> &rbeg = t.rbeg;
    const int64_t G = t.G, row_len = t.row_len;
    const int32_t R = t.R;
    c = HostChunking();
    c.seg_u.reserve((size_t)t.nnz); c.seg_w.reserve((size_t)t.nnz);
    // regions are ordered along latitude bands of `band_rows` grid rows (column-major inside a
    // band): a chunk then covers ~band_rows rows x a run of columns
    const int band_rows = knobs.band_rows;
    std::vector<int32_t> order;
    std::vector<double> key_col((size_t)R, 0.0);
    std::vector<int64_t> key_band((size_t)R, 0);
    for (int32_t r = 0; r < R; ++r) {
        const int64_t n = rbeg[(size_t)r + 1] - rbeg[(size_t)r];
        if (n == 0) { c.empty.push_back(r); continue; }
        double srow = 0, scol = 0;
        for (int64_t i = rbeg[(size_t)r]; i < rbeg[(size_t)r + 1]; ++i) {
            srow += (double)(segs[(size_t)i].cell / row_len);
            scol += (double)(segs[(size_t)i].cell % row_len);
        }
        key_band[(size_t)r] = (int64_t)(srow / (double)n) / band_rows;
        key_col[(size_t)r] = scol / (double)n;
        order.push_back(r);
    }
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        if (key_band[(size_t)a] != key_band[(size_t)b]) return key_band[(size_t)a] < key_band[(size_t)b];
        if (key_col[(size_t)a] != key_col[(size_t)b]) return key_col[(size_t)a] < key_col[(size_t)b];
        return a < b;
    });

    // greedy grouping on aligned 4-cell QUADS (16 bytes of a fp32 row): the kernel fetches
    // a chunk as up to UQ quads per timestep with one dwordx4 per lane
    struct Group { std::vector<int32_t> regions; int64_t n_q = 0, n_seg = 0; bool giant = false; };
    std::vector<Group> groups;
    std::vector<int32_t> stamp((size_t)(G + 3) / 4, -1);
    auto quads_of = [&](int32_t r) {       // distinct quads of a region (its cells are sorted)
        int64_t n = 0;
        int32_t last = -1;
        for (int64_t i = rbeg[(size_t)r]; i < rbeg[(size_t)r + 1]; ++i) {
            const int32_t q = segs[(size_t)i].cell >> 2;
            if (q != last) { ++n; last = q; }
        }
        return n;
    };
    Group cur;
    int32_t cur_id = 0;
    auto close = [&]() {
        if (!cur.regions.empty()) { groups.push_back(std::move(cur)); cur = Group(); }
        ++cur_id;
    };
    for (int32_t r : order) {
        const int64_t b = rbeg[(size_t)r], e = rbeg[(size_t)r + 1];
        const int64_t nq_r = quads_of(r);
        if (nq_r > UQ || e - b > SEG_MAX) {
            close();
            Group gg; gg.regions.push_back(r); gg.n_q = nq_r; gg.giant = true;
            groups.push_back(std::move(gg));
            ++c.n_giant;
            continue;
        }
        int64_t fresh = 0;
        {
            int32_t last = -1;
            for (int64_t i = b; i < e; ++i) {
                const int32_t q = segs[(size_t)i].cell >> 2;
                if (q != last) { fresh += stamp[(size_t)q] != cur_id; last = q; }
            }
        }
        if (cur.n_q + fresh > UQ || (int64_t)cur.regions.size() + 1 > RG_MAX ||
            cur.n_seg + (e - b) > SEG_MAX) {
            close();
            fresh = nq_r;
        }
        for (int64_t i = b; i < e; ++i) stamp[(size_t)(segs[(size_t)i].cell >> 2)] = cur_id;
        cur.n_q += fresh;
        cur.n_seg += e - b;
        cur.regions.push_back(r);
    }
    close();
    // giant groups (many chunks) first, largest first; all other groups stay in band/column
    // order so that consecutive workgroups touch neighbouring cells of the same grid rows
    std::stable_sort(groups.begin(), groups.end(), [](const Group &a, const Group &b) {
        if (a.giant != b.giant) return a.giant;
        return a.giant && a.n_q > b.n_q;
    });

    // flatten
    std::vector<int32_t> &pos = stamp;  // reuse as quad -> local index scratch
    std::vector<int32_t> quads;
    for (const Group &gr : groups) {
        c.grp_giant.push_back(gr.giant ? 1 : 0);
        if (gr.giant) {
            const int32_t r = gr.regions[0];
            const int64_t b = rbeg[(size_t)r], e = rbeg[(size_t)r + 1];
            int64_t cb = b;
            while (cb < e) {
                // take segments until the chunk holds UQ quads
                int64_t ce = cb, nq = 0;
                int32_t last = -1;
                const size_t ubase = c.ucell.size();
                while (ce < e) {
                    const int32_t q = segs[(size_t)ce].cell >> 2;
                    if (q != last) {
                        if (nq == UQ) break;
                        c.ucell.push_back(q * 4);
                        ++nq; last = q;
                    }
                    ++ce;
                }
                c.chunk_u_begin.push_back((int32_t)c.ucell.size());
                // split the chunk's segments over the waves
                const int64_t n = ce - cb, per = (n + NWAVE - 1) / NWAVE;
                for (int64_t sb = 0; sb < n; sb += per) {
                    const int64_t se = std::min<int64_t>(sb + per, n);
                    for (int64_t i = sb; i < se; ++i) {
                        const int32_t cell = segs[(size_t)(cb + i)].cell;
                        // local quad index: position of cell>>2 among this chunk's quads
                        const auto it = std::lower_bound(c.ucell.begin() + (std::ptrdiff_t)ubase, c.ucell.end(),
                                                         (cell >> 2) * 4);
                        c.seg_u.push_back((int32_t)((it - (c.ucell.begin() + (std::ptrdiff_t)ubase)) * 4 + (cell & 3)));
                        c.seg_w.push_back(segs[(size_t)(cb + i)].w);
                    }
                    c.ent_region.push_back(r);
                    c.ent_seg_begin.push_back((int32_t)c.seg_u.size());
                }
                c.chunk_e_begin.push_back((int32_t)c.ent_region.size());
                cb = ce;
            }
        } else {
            quads.clear();
            for (int32_t r : gr.regions)
                for (int64_t i = rbeg[(size_t)r]; i < rbeg[(size_t)r + 1]; ++i)
                    quads.push_back(segs[(size_t)i].cell >> 2);
            std::sort(quads.begin(), quads.end());
            quads.erase(std::unique(quads.begin(), quads.end()), quads.end());
            for (size_t i = 0; i < quads.size(); ++i) {
                pos[(size_t)quads[i]] = (int32_t)i;
                c.ucell.push_back(quads[i] * 4);
            }
            c.chunk_u_begin.push_back((int32_t)c.ucell.size());
            for (int32_t r : gr.regions) {
                for (int64_t i = rbeg[(size_t)r]; i < rbeg[(size_t)r + 1]; ++i) {
                    const int32_t cell = segs[(size_t)i].cell;
                    c.seg_u.push_back(pos[(size_t)(cell >> 2)] * 4 + (cell & 3));
                    c.seg_w.push_back(segs[(size_t)i].w);
                }
                c.ent_region.push_back(r);
                c.ent_seg_begin.push_back((int32_t)c.seg_u.size());
            }
            c.chunk_e_begin.push_back((int32_t)c.ent_region.size());
        }
        c.grp_chunk_begin.push_back((int32_t)(c.chunk_u_begin.size() - 1));
    }
}

// maximal runs of adjacent quads in a sorted list of distinct quads (first cells): run k = cells src[k] .. src[k] + len[k] - 1
static void quad_runs(const std::vector<int32_t> &uq, std::vector<int64_t> &src, std::vector<int32_t> &len) {
    src.clear(); len.clear();
    for (size_t i = 0; i < uq.size(); ++i) {
        if (i > 0 && uq[i] == uq[i - 1] + 4) len.back() += 4;
        else { src.push_back((int64_t)uq[i]); len.push_back(4); }
    }
}

void finish_chunking(HostChunking &c, bool lines, bool with_maps) {
    const std::vector<int32_t> &chunk_u_begin = c.chunk_u_begin, &chunk_e_begin = c.chunk_e_begin, &ent_seg_begin = c.ent_seg_begin;
    std::vector<int32_t> &seg_u = c.seg_u, &ucell = c.ucell;
    // bit 15 of a segment's local cell index marks the LAST segment of its region entry
    // (local indices are < 256); entries without segments cannot exist (every entry has >= 1)
    for (size_t e = 0; e + 1 < ent_seg_begin.size(); ++e)
        if (ent_seg_begin[e + 1] > ent_seg_begin[e]) seg_u[(size_t)ent_seg_begin[e + 1] - 1] |= SEG_LAST;
    // bits 16..23: index of the segment's entry inside its chunk (read by the MFMA kernel)
    for (size_t k = 0; k + 1 < chunk_e_begin.size(); ++k)
        for (int32_t e = chunk_e_begin[k]; e < chunk_e_begin[k + 1]; ++e)
            for (int32_t q = ent_seg_begin[(size_t)e]; q < ent_seg_begin[(size_t)e + 1]; ++q)
                seg_u[(size_t)q] |= (e - chunk_e_begin[k]) << 16;
    // per-chunk descriptors for the persistent kernel; giant groups come first.  dd[6] packs the
    // entry split points of the four waves (contiguous entry ranges with ~equal segment counts)
    c.chunk_desc.assign((size_t)(chunk_u_begin.size() - 1) * 8, 0);
    for (size_t k = 0; k + 1 < chunk_u_begin.size(); ++k) {
        int32_t *dd = &c.chunk_desc[k * 8];
        dd[0] = chunk_u_begin[k]; dd[1] = chunk_u_begin[k + 1] - chunk_u_begin[k];
        dd[2] = chunk_e_begin[k]; dd[3] = chunk_e_begin[k + 1] - chunk_e_begin[k];
        dd[4] = ent_seg_begin[(size_t)chunk_e_begin[k]];
        dd[5] = ent_seg_begin[(size_t)chunk_e_begin[k + 1]] - dd[4];
        int32_t split[SWAVE + 1];
        for (int i = 0; i <= SWAVE; ++i) split[i] = i == SWAVE ? dd[3] : 0;
        int w = 1;
        for (int32_t e = 0; e < dd[3] && w < SWAVE; ++e) {
            const int64_t done = ent_seg_begin[(size_t)(dd[2] + e + 1)] - dd[4];
            while (w < SWAVE && done * SWAVE >= (int64_t)dd[5] * w) split[w++] = e + 1;
        }
        while (w < SWAVE) split[w++] = dd[3];
        uint64_t packed = 0;
        for (int i = 1; i < SWAVE; ++i) packed |= (uint64_t)(split[i] & 0xff) << (8 * (i - 1));
        dd[6] = (int32_t)(uint32_t)(packed & 0xffffffffu);
        dd[7] = (int32_t)(uint32_t)(packed >> 32);
    }
    c.g0_normal = 0;
    while (c.g0_normal < (int)c.grp_giant.size() && c.grp_giant[(size_t)c.g0_normal]) ++c.g0_normal;
    c.c0_normal = c.grp_chunk_begin[(size_t)c.g0_normal];

    c.lines128 = c.sectors64 = 0;
    for (size_t k = 0; k + 1 < chunk_u_begin.size(); ++k) {      // locality statistics of the gather
        int32_t l128 = -1, s64 = -1;
        std::vector<int32_t> qs(ucell.begin() + chunk_u_begin[k], ucell.begin() + chunk_u_begin[k + 1]);
        std::sort(qs.begin(), qs.end());
        for (int32_t q : qs) {
            if ((q >> 5) != l128) { l128 = q >> 5; ++c.lines128; }
            if ((q >> 4) != s64) { s64 = q >> 4; ++c.sectors64; }
        }
    }
    if (!(lines && with_maps)) return;
    // Whole-line chunkings: which quads of a chunk does a segment really read?  A chunk fetches every quad of its lines; the
    // others are parked in the image and never read -- except quad 0, whose first cell the padding lanes of the consumers
    // read with weight 0 (so it counts as referenced: its data must be sane for 0 * x = 0).  Unreferenced quads get bit 0 of
    // their ucell entry set (UCELL_UNREF; quads are 4-cell aligned, the low bits are free): the kernels mask it off the address,
    // and sparse_lcv_kernel leaves what such a quad loads out of its finite / general decision (Regs::unref).
    // (a segment's local cell index is the low byte of seg_u -- bit 15 and bits 16..23 carry flags by now, see above)
    std::vector<char> used(ucell.size(), 0);
    bool map_ok = true;
    for (size_t k = 0; k + 1 < chunk_u_begin.size() && map_ok; ++k) {
        const int32_t nq = chunk_u_begin[k + 1] - chunk_u_begin[k];
        if (nq > 0) used[(size_t)chunk_u_begin[k]] = 1;
        for (int32_t e = chunk_e_begin[k]; e < chunk_e_begin[k + 1] && map_ok; ++e)
            for (int32_t sg = ent_seg_begin[(size_t)e]; sg < ent_seg_begin[(size_t)e + 1]; ++sg) {
                const int32_t q = (seg_u[(size_t)sg] & 0xff) >> 2;
                if (q >= nq) { map_ok = false; break; }                  // (cannot happen; then: no flags, no quad map)
                used[(size_t)chunk_u_begin[k] + (size_t)q] = 1;
            }
    }
    if (map_ok)
        for (size_t i = 0; i < ucell.size(); ++i) if (!used[i]) ucell[i] |= UCELL_UNREF;
    // the compact row of the lines-only host path: the distinct quads of this chunking in grid order, side by side
    // (ucell entries carry UCELL_UNREF in bit 0: compared without it, handed on with it)
    std::vector<int32_t> uq(ucell.size());
    for (size_t i = 0; i < ucell.size(); ++i) uq[i] = ucell[i] & ~UCELL_UNREF;
    std::sort(uq.begin(), uq.end());
    uq.erase(std::unique(uq.begin(), uq.end()), uq.end());
    c.ucell_c.resize(ucell.size());
    for (size_t i = 0; i < ucell.size(); ++i)
        c.ucell_c[i] = (int32_t)(4 * (std::lower_bound(uq.begin(), uq.end(), ucell[i] & ~UCELL_UNREF) - uq.begin())) | (ucell[i] & UCELL_UNREF);
    quad_runs(uq, c.run_src, c.run_len);
    c.Gc = 4 * (int64_t)uq.size();
    // ... and the quads that count as referenced only (wagg_sparse_int.h: ucell_q); the others point at position 0 of
    // the row (any valid address: what they load is neither read nor counted)
    if (!map_ok) return;
    std::vector<int32_t> uqq;
    for (size_t i = 0; i < ucell.size(); ++i) if (used[i]) uqq.push_back(ucell[i]);
    std::sort(uqq.begin(), uqq.end());
    uqq.erase(std::unique(uqq.begin(), uqq.end()), uqq.end());
    c.ucell_q.assign(ucell.size(), UCELL_UNREF);
    for (size_t i = 0; i < ucell.size(); ++i)
        if (used[i]) c.ucell_q[i] = (int32_t)(4 * (std::lower_bound(uqq.begin(), uqq.end(), ucell[i]) - uqq.begin()));
    quad_runs(uqq, c.run_src_q, c.run_len_q);
    c.Gq = 4 * (int64_t)uqq.size();
}

}  // namespace wagg
