// Host chunking of a segment table: the stages between a caller's (cell, region, weight) rows and the arrays a
// SparsePlanDev is uploaded from.  Plain C++17 and std::vector -- no HIP, no plan object, no environment: wagg_sparse.hip
// runs the stages and uploads what they return; tests/chunk_dump.cpp links this unit alone.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace wagg {

// LDS / chunk geometry shared by the builder and the kernels (wagg_sparse_int.h includes this header)
constexpr int UC = 256;      // cell slots per LDS chunk == workgroup size
constexpr int UQ = UC / 4;   // aligned 4-cell quads per chunk (one per lane of a wave)
constexpr int RG_MAX = 127;  // regions per group
constexpr int SEG_MAX = 512; // segments per chunk staged in LDS
constexpr int UCELL_UNREF = 1;     // bit 0 of a ucell entry of a WHOLE-LINE chunking: the quad holds no referenced cell (finish_chunking)
constexpr int SEG_LAST = 0x8000;   // flag bit in a segment's local cell index: last segment of its entry
constexpr int SEG_UMASK = 0x7fff;
constexpr int NWAVE = 4;      // waves of the chunk-walking kernel (256 threads)
constexpr int SWAVE = 8;      // waves of the persistent stream kernel (512 threads)

struct Seg { int32_t region, cell; double w; };

// the coalesced table: one row per kept (region, cell) pair
struct SegTable {
    std::vector<Seg> segs;          // by (region, cell)
    std::vector<double> den;        // [R] sum of the kept weights of a region, in row order (aggregations.py:79)
    std::vector<int64_t> rbeg;      // [R + 1] region r owns segs[rbeg[r] .. rbeg[r + 1])
    int64_t nnz = 0;                // == segs.size()
    int64_t G = 0, row_len = 0;
    int32_t R = 0;
};

// why a table was refused: `code` is a WAGG_E* status (include/wagg.h), 0 = none; `text` goes to set_error as it is
struct ChunkError { int code = 0; std::string text; };

// the range checks of one row (region_code < R, 0 <= cell_idx < G), in that order; false + `err` when one fails
bool row_in_range(int64_t i, int32_t region, int32_t cell, int64_t G, int32_t R, ChunkError &err);

// rows -> SegTable: drops null labels (S3) and NaN weights, checks the others, sorts by (region, cell) and adds up duplicate
// pairs in table order (S5).  `row_len` must be in [1, G].  false + `err` on a row out of range.
bool coalesce_table(const int32_t *cell_idx, const int32_t *region_code, const double *w_eff, int64_t nseg, int64_t G, int32_t R,
                    int64_t row_len, SegTable &t, ChunkError &err);

// whole-line chunkings exist for a grid of whole rows of whole quads with at least one kept row
inline bool lines_applicable(const SegTable &t) {
    return t.row_len < t.G && t.G % t.row_len == 0 && t.row_len % 4 == 0 && t.nnz > 0;
}

// diagnostic-build values (wagg_sparse.hip reads them from the environment; the production library passes the defaults)
struct ChunkKnobs {
    int band_rows = 8;       // grid rows per latitude band of the region-shaped chunks
    int lines_order = 0;     // 2: whole-line chunks in band-major order instead of strip-major
};

// one chunking of a table, as host vectors (the names are SparsePlanDev's)
struct HostChunking {
    std::vector<int32_t> grp_chunk_begin{0}, grp_giant, chunk_u_begin{0}, chunk_e_begin{0};
    std::vector<int32_t> ucell, ent_region, ent_seg_begin{0}, seg_u;   // ucell = first cell of each quad
    std::vector<double> seg_w;
    std::vector<int32_t> empty;                                        // regions without any kept row
    std::vector<int32_t> chunk_desc;                                   // [n_chunks][8]
    std::vector<int32_t> part_begin;                                   // whole-line chunking only
    int64_t n_part_rows = 0;
    int g0_normal = 0, c0_normal = 0;
    int64_t n_giant = 0;
    // whole-line chunkings finished `with_maps`: the compact rows of the host paths (wagg_sparse_int.h: ucell_c, ucell_q)
    std::vector<int32_t> ucell_c, ucell_q;
    std::vector<int64_t> run_src, run_src_q;
    std::vector<int32_t> run_len, run_len_q;
    int64_t Gc = 0, Gq = 0;
    int64_t lines128 = 0, sectors64 = 0;                               // locality statistics of the gather
};

// whole lines of `line_cells` cells, `lines_per_chunk` to a chunk; false (and `c` unspecified) where the form does not apply
bool chunk_lines(const SegTable &t, int line_cells, int lines_per_chunk, const ChunkKnobs &knobs, HostChunking &c);
// region-shaped chunks: always apply
void chunk_regions(const SegTable &t, const ChunkKnobs &knobs, HostChunking &c);
// flag bits of seg_u, chunk descriptors, g0_normal / c0_normal, locality statistics; for a whole-line chunking (`lines`)
// `with_maps` adds the UCELL_UNREF marks and both compact maps with their runs
void finish_chunking(HostChunking &c, bool lines, bool with_maps);

}  // namespace wagg
