// Which launches one apply of a full-form or tile-sparse dense plan runs, and how large their workspaces are: the row groups
// of a batch, the k-split, the form of each launch and its pack-free first pass, decided from a handful of plan and call
// scalars.  Also the plan-time choice between the three forms.  Plain C++ -- no HIP, no plan object, no environment reads,
// no allocation, O(1) per call: dense_apply (wagg_dense.hip) asks and launches what the answer says;
// tests/dense_route_dump.cpp links this unit alone and enumerates it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace wagg {

// ---- the row-block heights MT (x 16 rows) the kernels are instantiated for: the ONLY list.  The lookup below and every
// kernel switch of wagg_dense.hip (WAGG_PICK) are generated from it, so an MT handed out here always has its kernels.
#define WAGG_DENSE_MTS_F32(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(21) X(22) X(23)
#define WAGG_DENSE_MTS_F64(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(10) X(11)
#define WAGG_DENSE_MT_ITEM(M) M,
constexpr int DENSE_MTS_F32[] = {WAGG_DENSE_MTS_F32(WAGG_DENSE_MT_ITEM)};
constexpr int DENSE_MTS_F64[] = {WAGG_DENSE_MTS_F64(WAGG_DENSE_MT_ITEM)};
#undef WAGG_DENSE_MT_ITEM
constexpr int DENSE_N_MTS_F32 = (int)(sizeof(DENSE_MTS_F32) / sizeof(int)), DENSE_N_MTS_F64 = (int)(sizeof(DENSE_MTS_F64) / sizeof(int));
// the lists ascend: the last entry is the tallest workgroup (the accumulators of 23 / 11 row blocks fill the register file)
constexpr int DENSE_MT_MAX_F32 = DENSE_MTS_F32[DENSE_N_MTS_F32 - 1], DENSE_MT_MAX_F64 = DENSE_MTS_F64[DENSE_N_MTS_F64 - 1];
constexpr int dense_mt_max(int elem) { return elem == 8 ? DENSE_MT_MAX_F64 : DENSE_MT_MAX_F32; }
// full form, pack-free: instantiated for the tall row blocks only (fp32 MT >= 20, fp64 MT >= 10), where the packing pass is
// worth skipping
constexpr bool dense_full_pack_free_mt(int elem, int MT) { return elem == 8 ? MT >= 10 : MT >= 20; }

constexpr int DENSE_BN = 256;                // columns of a W tile (8 waves x 32)
constexpr int DENSE_ROWB = 128;              // bytes of one tile row: 32 floats or 16 doubles of k
constexpr int dense_bk(int elem) { return DENSE_ROWB / elem; }

// the smallest MT of the set with 16 MT >= rows (the tallest when none holds them)
int dense_pick_mt(int elem, int64_t rows);

// Long batches (ensemble x time rows of a small grid: 50 members x 30 years = 547,500 rows) go through in groups of
// whole row blocks: the reduce kernel's grid has one y block per row (<= 65,535), and the packed copy of X and the
// partial slabs are sized by the rows of one launch.  Same stream, same workspaces, one group after the other.
constexpr int64_t dense_rows_max(int elem) { return (int64_t)(65535 / (dense_mt_max(elem) * 16)) * (dense_mt_max(elem) * 16); }

// one launch: rows [row0, row0 + rows) of the batch as n_mb row blocks of MT x 16 rows
struct DenseRowGroup { int64_t row0 = 0, rows = 0; int MT = 0, n_mb = 0; };
struct DenseRowGroups { int n = 0; DenseRowGroup g[2]; };
// the one or two launches of Tn <= dense_rows_max(elem) rows
DenseRowGroups dense_row_groups(int elem, int64_t Tn);

int pick_ksplit(int64_t items, int n_kt);

struct DensePlanScalars {
    int elem = 4;                           // bytes of an element
    int n_nt = 0, n_kt = 0;                 // column tiles (256 regions), k tiles (32 / 16 cells)
    int64_t G = 0;
    bool tiled = false, spmm = false;
    bool has_maxima = false;                // full-form fp32 plans: the column maxima the split form scales by
    bool has_image = false;                 // ... and the f16 hi/lo image of W
};
struct DenseCall {
    int MT = 0, n_mb = 0;                   // of the row group (dense_row_groups)
    int64_t rows = 0;
    int ksplit = 0;                         // the caller's: 0 = pick_ksplit
    bool exact = false;                     // WAGG_APPLY_EXACT_F32
    int xf_mode = 0;                        // PackXfT::mode: 0 = plain aggregation
    bool aligned16 = false;                 // X (degree days: and X2) and the row pitch are 16-byte aligned
    bool nonfinite_met = false;             // an earlier pack-free pass of this plan met NaN / +-inf
};

enum { DENSE_FORM_NONE = 0, DENSE_FORM_SPLIT = 1, DENSE_FORM_FULL = 2, DENSE_FORM_TILED = 3 };   // NONE: an entry-list plan (spmm_apply)
enum { PACK_FREE_NONE = 0, PACK_FREE_TILED = 1, PACK_FREE_FULL = 2 };

struct DenseRoute {
    int form = DENSE_FORM_NONE;
    int S = 0, kt_per_slice = 0;            // k-slices (tile-sparse: 1, the launch walks pieces) and k tiles per slice
    bool image = false;                     // split form: W comes from the plan's image (launches of ONE row block)
    // the first pass that reads X where it lies; PACK_FREE_FULL: the second pass is the gated packed kernel
    int pack_free = PACK_FREE_NONE;
    int64_t nblk = 0;                       // workgroups = slabs of the launch; tile-sparse: 0 (tile_pieces_for has both)
    int64_t x_slots = 0;                    // 16-byte slots of the packed X
    // workspaces in 4-byte words (DevBuf<float>): one slab, all nblk of them, the packed X, the row maxima (split form)
    size_t slab_words = 0, slabs_words = 0, xp_words = 0, xmax_words = 0;
};
DenseRoute dense_launch_route(const DensePlanScalars &p, const DenseCall &c);
// the route of the plan's largest launch group (one row block of MT_MAX x 16 rows at pick_ksplit's S): what
// dense_build_image sizes the workspaces by
DenseRoute dense_largest_group_route(const DensePlanScalars &p);

// Generated tables (wagg_dense_create_synth*): below this share of non-zeros a scattered W goes to the entry-list form.
constexpr double SPMM_MAX_FILL = 0.10;

// ---- which form a caller's table takes (wagg_dense_create_from_csr* / _from_segments*) ---------------------------------
// The reference knows one weights type (aggregations.py:64-73) and so does the caller here: the form is the library's
// business.  It is chosen by the estimated time per row of X of the three forms, each priced at the rate its kernel was
// MEASURED at on the c5 grid (tools/form_crossover.py -> profiles/r05_form_crossover.txt; docs/HISTORY.md (b) has the table):
//   full matrix     2 x (all tiles x BK x 256) flop     at the full-form MFMA rate (padding of G and R to whole tiles included)
//   tile-sparse     2 x (stored tiles x BK x 256) flop  at the tile-sparse MFMA rate (a little lower: the tile list is walked)
//   entry lists     2 x walked entries flop at the entry-loop rate of their mean list length, but never faster than the X
//                   stream that every one of the n_rb region blocks pulls through the LDS-DMA path (b G n_rb bytes per row)
// Rates in flop/s and byte/s; fp32 / fp64.
struct FormRates { double full, tiled, entries_scale, dma; };
// fp32: full 204.3 ms for 2,282 rows x 8,100 x 96 tiles on the fp32 pipe (142 TF), since the split form (f16 pipe, row maxima
// and split pack included) 2.99x that: c2-dense 42.6 against 127.3 ms a step on one box, A/B -> 420 TF (re-derived for the
// W-in-registers pipeline from the form guard's forced full-form times, 424-446 TF, then 445-470 TF: kept); tile-sparse (a
// workgroup walks an equal share of the stored tiles: dense_pieces_kernel) 144 TF on the stored tiles' flops (c5-block:
// 8.39 ms), fp64 73 TF (16.58 ms); c5-uniform-f64 of bench.py for the fp64 entry-list scale
constexpr FormRates FORM_RATES_F32 = {420e12, 144e12, 1.0, 10.1e12};
constexpr FormRates FORM_RATES_F64 = {70e12, 73e12, 0.44, 10.1e12};
double entry_loop_rate(double mean_list);

struct FormCost { double t_full, t_tiled, t_entries; };
FormCost table_form_cost(int64_t G, int elem_bytes, int64_t n_tiles_stored, int64_t n_tiles_all, int64_t walked, int n_rb,
                         int64_t n_lists, int n_nt);
void pick_table_form(const FormCost &c, bool *tiled, bool *entries);

}  // namespace wagg
