// The schedule of a dense apply and the plan-time form choice (wagg_dense_route.h).  Plain C++: no HIP header, nothing allocated.
#include "wagg_dense_route.h"

#include <cmath>

namespace wagg {

int dense_pick_mt(int elem, int64_t rows) {
    const int *mts = elem == 8 ? DENSE_MTS_F64 : DENSE_MTS_F32;
    const int n = elem == 8 ? DENSE_N_MTS_F64 : DENSE_N_MTS_F32;
    for (int i = 0; i < n; ++i)
        if ((int64_t)mts[i] * 16 >= rows) return mts[i];
    return mts[n - 1];
}

// row blocks: as few as possible (<= MT_MAX x 16 rows each), evenly filled, 16 MT rows with MT from the
// instantiated set -- fp32: T = 365 -> one block of 23 x 16; T = 1369 -> four of 22 x 16; T = 31 -> 2 x 16
DenseRowGroups dense_row_groups(int elem, int64_t Tn) {
    DenseRowGroups out;
    const int bm_max = dense_mt_max(elem) * 16;
    const int n_mb = (int)((Tn + bm_max - 1) / bm_max);
    const int MT = dense_pick_mt(elem, (Tn + n_mb - 1) / n_mb);
    // A ragged batch: with equal row blocks the padding of EVERY block is paid (c4's rank shard: 1,369 rows = 4 x 343 -> 4 blocks
    // of 22 x 16 = 1,408 rows, 2.8 % of the MFMA work on zero rows).  Full blocks first, the remainder as a launch of its own with
    // the smallest row-block count that holds it (3 x 352 + 313 -> 22, 22, 22, 20: 1,376 rows) -- when that saves at least two
    // sixteen-row units and the remainder is tall enough to stay MFMA-bound against its own pass over W.
    if (n_mb >= 2) {
        const int64_t head = (int64_t)(n_mb - 1) * MT * 16, tail = Tn - head;
        const int MT_tail = dense_pick_mt(elem, tail);
        if (tail > 0 && MT_tail >= 4 && MT - MT_tail >= 2) {
            out.n = 2;
            out.g[0].row0 = 0; out.g[0].rows = head; out.g[0].MT = MT; out.g[0].n_mb = n_mb - 1;
            out.g[1].row0 = head; out.g[1].rows = tail; out.g[1].MT = MT_tail; out.g[1].n_mb = 1;
            return out;
        }
    }
    out.n = 1;
    out.g[0].row0 = 0; out.g[0].rows = Tn; out.g[0].MT = MT; out.g[0].n_mb = n_mb;
    return out;
}

int pick_ksplit(int64_t items, int n_kt) {
    int best = 8;
    double best_eff = 0.0;
    for (int S = 8; S <= 64; S += 8) {
        if (S > 8 && n_kt / S < 32) break;             // keep >= 32 LDS tiles per slice
        const double w = (double)items * S / 256.0;
        const double eff = w / std::ceil(w);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = S; }
        if (eff >= 0.985) break;
    }
    return best;
}

DenseRoute dense_launch_route(const DensePlanScalars &p, const DenseCall &c) {
    DenseRoute r;
    if (p.spmm) return r;
    const size_t bm = (size_t)c.MT * 16;
    r.S = c.ksplit ? c.ksplit : pick_ksplit((int64_t)p.n_nt * c.n_mb, p.n_kt);
    r.x_slots = (int64_t)c.n_mb * p.n_kt * (int64_t)bm * 8;
    r.xp_words = (size_t)r.x_slots * 4;
    r.slab_words = bm * DENSE_BN * (size_t)(p.elem / 4);
    // fp32 full form: the split form unless the caller asked for the exact kernel (WAGG_APPLY_EXACT_F32)
    if (p.elem == 4 && !p.tiled && !c.exact && p.has_maxima) {
        r.form = DENSE_FORM_SPLIT;
        // the image serves launches of ONE row block.  With several, every W tile is contracted once per row block and all but
        // the first read are L2 hits; there the image measured no gain (c4's share, four row blocks: 0.6 % slower in every
        // alternation, profiles/split_image_ab.txt), so those launches split in registers as before.
        r.image = p.has_image && c.n_mb == 1;
        r.xmax_words = (size_t)c.rows;
    } else {
        // tile-sparse form: no k-slices -- the launch walks PIECES, an equal share of all stored tiles per workgroup (see the kernel)
        r.form = p.tiled ? DENSE_FORM_TILED : DENSE_FORM_FULL;
        if (p.tiled) r.S = 1;
        // pack-free first pass (plain aggregation of 16-byte-aligned rows, grid = whole k tiles):
        // the MFMA kernel reads X where it lies; the packed pass then runs only if a numerator came out
        // non-finite (NaN / +-inf somewhere in the data), gated on the device so the stream never waits for the host
        // ... and only while no earlier pack-free pass of this plan met such data: fields with NaN in them (ocean cells of
        // land-only variables) tend to stay that way, and for them the first pass is pure overhead.
        // (G must be a whole number of k tiles: the last tile is then read from inside every row, whatever the caller's
        // pitch and however short the buffer behind the last row is)
        const bool rm = c.xf_mode == 0 && c.aligned16 && p.G % dense_bk(p.elem) == 0 && !c.nonfinite_met;
        if (rm && p.tiled) r.pack_free = PACK_FREE_TILED;
        // (full form: only with two or more row blocks -- with one, A/B on one GPU shows the step unchanged: the kernel
        // loses reading in place what the skipped packing pass saves)
        else if (rm && c.n_mb >= 2 && dense_full_pack_free_mt(p.elem, c.MT)) r.pack_free = PACK_FREE_FULL;
    }
    r.kt_per_slice = (p.n_kt + r.S - 1) / r.S;
    if (!p.tiled) {
        r.nblk = (int64_t)p.n_nt * c.n_mb * r.S;
        r.slabs_words = (size_t)r.nblk * r.slab_words;
    }
    return r;
}

DenseRoute dense_largest_group_route(const DensePlanScalars &p) {
    DenseCall c;
    c.MT = dense_mt_max(p.elem); c.n_mb = 1; c.rows = (int64_t)c.MT * 16;
    return dense_launch_route(p, c);
}

// The entry loop slows down as the lists grow (the first 16 groups of a wave's list are preloaded across the previous chunk;
// what follows is fetched inside the loop): flop/s on the WALKED entries against the mean list length per wave and chunk,
// fp32, measured at uniform fills of 1, 3, 6, 10, 15 and 30 % (mean lengths 54 ... 1625)
double entry_loop_rate(double mean_list) {
    static const double L[] = {170, 325, 541, 812, 1625}, Rt[] = {30e12, 23e12, 19.5e12, 17.3e12, 15.9e12};
    if (mean_list <= L[0]) return Rt[0];
    for (int i = 1; i < 5; ++i)
        if (mean_list <= L[i]) return Rt[i - 1] + (Rt[i] - Rt[i - 1]) * (mean_list - L[i - 1]) / (L[i] - L[i - 1]);
    return Rt[4];
}

// seconds per row of X.  The MFMA forms multiply whole (BK x 256) tiles, padding included; the entry-list kernel walks
// `walked` entries (spmm_list_cost: 16 x the longest per-wave list of every item, in whole groups) spread over n_lists
// (region block, chunk, wave) lists.
FormCost table_form_cost(int64_t G, int elem_bytes, int64_t n_tiles_stored, int64_t n_tiles_all, int64_t walked, int n_rb,
                         int64_t n_lists, int n_nt) {
    const FormRates &rt = elem_bytes == 8 ? FORM_RATES_F64 : FORM_RATES_F32;
    const double tile_flop = 2.0 * (128.0 / elem_bytes) * 256.0;        // BK = 32 / 16 cells x 256 regions
    FormCost c;
    // (full form with few column tiles: a launch has at most n_nt x 64 k-slices of workgroups per row block -- R = 600 fills
    //  192 of 256 CUs; the tile-sparse form hands every CU an equal share of the stored tiles whatever their layout)
    // (pick_ksplit keeps >= 32 k tiles per slice: a short K has fewer than 64 slices -- G = 700: 8 -- and at the split form's
    //  rate that, not the MFMA pipe, is what a small full-form launch is paid by)
    const int64_t n_kt = n_tiles_all / (n_nt > 0 ? n_nt : 1);
    const double s_max = n_kt / 32 >= 64 ? 64.0 : (n_kt / 32 >= 16 ? (double)(n_kt / 32 / 8 * 8) : 8.0);
    const double util = n_nt * s_max < 256.0 ? n_nt * s_max / 256.0 : 1.0;
    c.t_full = tile_flop * (double)n_tiles_all / (rt.full * util);
    c.t_tiled = tile_flop * (double)n_tiles_stored / rt.tiled;
    const double rate = rt.entries_scale * entry_loop_rate((double)walked / (double)(n_lists > 0 ? n_lists : 1));
    const double t_loop = 2.0 * (double)walked / rate, t_stream = (double)elem_bytes * (double)G * (double)n_rb / rt.dma;
    c.t_entries = t_loop > t_stream ? t_loop : t_stream;
    return c;
}
void pick_table_form(const FormCost &c, bool *tiled, bool *entries) {
    *entries = c.t_entries < c.t_full && c.t_entries < c.t_tiled;
    *tiled = !*entries && c.t_tiled < c.t_full;
}

}  // namespace wagg
