// Internal declarations of the segment-table path shared by wagg_sparse.hip and -- in the diagnostic build --
// wagg_sparse_diag.hip: the plan object, the device views the kernels take, the LDS geometry constants.
#pragma once
#include <mutex>
#include <vector>

#include "wagg_chunk.h"
#include "wagg_host.h"
#include "wagg_route.h"

namespace wagg {

// Diagnostic knobs (ablation switches, phase stamps) exist only in the -DWAGG_DIAG build
// (`make diag` -> libwagg_diag.so, used by tools/*_ablate.sh); the production library reads no
// environment variable on any path.
#ifdef WAGG_DIAG
static inline int diag_env(const char *name) { const char *v = getenv(name); return v ? atoi(v) : 0; }
static inline bool diag_set(const char *name) { return getenv(name) != nullptr; }
#else
static inline constexpr int diag_env(const char *) { return 0; }
static inline constexpr bool diag_set(const char *) { return false; }
#endif

// (UC, UQ, RG_MAX, SEG_MAX, NWAVE, SWAVE and the seg_u / ucell flag bits: wagg_chunk.h)
[[maybe_unused]] constexpr int UROW = UC + 4; // LDS row stride in elements (t-major image, 16-byte aligned rows): fp32, 260 dwords = 4 (mod 64)
// the same for a type: fp64 rows of UC + 2 doubles are 516 dwords = 4 (mod 64) as well (UC + 4 doubles = 8 (mod 64) made a
// lane = timestep column read 4-way conflicted: VERDICT r2 item 5); still 16-byte aligned for the vector stores
template <typename T> constexpr int urow() { return sizeof(T) == 8 ? UC + 2 : UC + 4; }
constexpr int STHREADS = SWAVE * 64;

struct SparsePlanDev {
    DevBuf<int32_t> grp_chunk_begin, grp_giant;   // [n_groups+1], [n_groups]
    DevBuf<int32_t> chunk_u_begin, chunk_e_begin; // [n_chunks+1]
    DevBuf<int32_t> ucell;                        // [n_ucells]
    DevBuf<int32_t> ent_region, ent_seg_begin;    // [n_ent], [n_ent+1]
    DevBuf<int32_t> seg_u;                        // [nnz]
    DevBuf<float> seg_w32;
    DevBuf<double> seg_w64;
    DevBuf<float> den32;
    DevBuf<double> den64;
    DevBuf<int32_t> empty_regions;
    DevBuf<int32_t> chunk_desc;
    DevBuf<float> ent_den32;
    DevBuf<double> ent_den64;
    int g0_normal = 0, c0_normal = 0;
    // whole-line plan: an entry is a (chunk, region) PARTIAL sum, ent_region its row in the partial buffer;
    // region r is the sum of rows part_begin[r] .. part_begin[r + 1] - 1 of the partial buffer, divided by den[r]
    DevBuf<int32_t> part_begin;
    int64_t n_part = 0;
    int64_t n_groups = 0, n_empty = 0;          // groups of this chunking; regions without any kept row
    // whole-line chunkings of (time, gridcell) data only -- the COMPACT row of the "lines only" host path (wagg_host.h,
    // WAGG_HOST_LINES): the distinct quads the chunks fetch, in grid order, packed side by side.  ucell_c[i] = position of
    // quad ucell[i] in that row; run k of the row = cells run_src[k] .. run_src[k] + run_len[k] - 1 of the grid row (maximal
    // runs of adjacent quads); Gc = cells of the compact row (0: no compact row)
    DevBuf<int32_t> ucell_c;
    std::vector<int64_t> run_src;
    std::vector<int32_t> run_len;
    int64_t Gc = 0;
    // the same at QUAD granularity (round 6, "quads only"): a whole-line chunk fetches every quad of its lines, but only the
    // quads that hold a referenced cell matter -- the others are loaded into the LDS image and never read.  ucell_q[i] = position
    // in the quad-compact row of quad ucell[i] if a segment of its chunk reads it (or it is the chunk's quad 0, which the
    // consumers' padding lanes read with weight 0), else position 0 with UCELL_UNREF set (any valid address: the value is neither
    // read nor counted); run_src_q / run_len_q / Gq as above for those quads only.  c2-real: ~35 % of a fp32 row where the whole
    // lines are 63.6 %.  Same kernel, same cells in the same order, the same finite / general decisions: the same bits.
    DevBuf<int32_t> ucell_q;
    std::vector<int64_t> run_src_q;
    std::vector<int32_t> run_len_q;
    int64_t Gq = 0;
};
// (COMPACT_NONE / COMPACT_LINES / COMPACT_QUADS, which row launch_sparse is handed: wagg_route.h)

// What a many-plan (wagg_plan_create_many) adds: K weightings of one table and n_levels coarse levels derived from the fine
// one.  The weightings are K plans built from the same kept rows (a row another weighting keeps has weight 0 where this one is
// NaN), so their chunkings are the same structure and only the segment weights and denominators differ; the kernels read the
// structure of weighting 0.  Coarse region c of a level is the sum of the partial rows in cpart_idx[cpart_begin[c] ..
// cpart_begin[c + 1]) of a whole-line chunking (the rows of its fine regions in fine-code order), divided by its den.
constexpr int MANY_MAX_W = 4, MANY_MAX_LEVELS = 3;
struct ManyLevel {
    int32_t R = 0;
    std::vector<int32_t> fine_to_coarse;             // [R fine] coarse code, -1: the fine region has no kept row
    std::vector<std::vector<double>> den;            // [K][R] fp64, row order (= wagg_plan_get_den of a plan over the coarse codes)
    DevBuf<float> den32[MANY_MAX_W];                 // [K] device copies
    DevBuf<double> den64[MANY_MAX_W];
    DevBuf<int32_t> cpart_begin32, cpart_idx32;      // over the partial rows of the fp32 whole-line chunking (dl)
    DevBuf<int32_t> cpart_begin64, cpart_idx64;      // ... of the fp64 one (dl64)
};

}  // namespace wagg

struct wagg_plan {
    wagg_plan_info info{};
    std::vector<double> den_host;
    wagg::SparsePlanDev d;        // region-shaped chunks: every kernel, every layout and data type
    wagg::SparsePlanDev dl;       // whole-line chunks (has_lines): 8 lines x 32 cells, the fp32 (time, gridcell) loader/consumer
    bool has_lines = false;       // kernel, which is bound by line requests
    wagg::SparsePlanDev dl64;     // the same for fp64 data: 8 lines x 16 cells (a line = 128 bytes of a row in both)
    bool has_lines64 = false;
    wagg::SparsePlanDev dl64e;    // 4 lines x 16 cells: fp64 degree days (both fields of a 64-cell chunk fill one image row)
    bool has_lines64e = false;
    int device = 0;
    int ncu = 256;                 // compute units of `device` (read once, at plan creation)
    int flags = 0;                 // WAGG_PLAN_* kernel-form switches, fixed at plan creation
    // set by a kernel whose consumer-wave barrier timed out (host-mapped, so the host can read it
    // without touching the stream); checked by the next apply, wagg_plan_status and the *_host_ forms
    int *timeout_host = nullptr, *timeout_dev = nullptr;
    // many-plans only (wagg_plan_create_many): `many_w[k]` = the plan of weighting k (owned); this handle's info.R is the width
    // of the concatenated result (out_cols) and den_host its denominators in that order; its own chunkings stay empty
    std::vector<wagg_plan *> many_w;
    wagg::ManyLevel many_lv[wagg::MANY_MAX_LEVELS];
    int many_nlv = 0;
    int32_t many_R0 = 0;
    // wagg_pack.hip: the first cell of every quad of the quads-only compact row, in row order (Gq / 4 entries), of the fp32
    // chunking `dl` ([0]) and the fp64 one `dl64` ([1]); uploaded by the first pack of that element type, freed with the plan
    mutable std::mutex pack_mu;
    mutable wagg::DevBuf<int32_t> pack_quads[2];
    mutable bool pack_ready[2] = {false, false};
    bool is_many() const { return !many_w.empty(); }
    int64_t many_col(int level, int k) const {       // first column of plane (level, k): level-major, then weighting
        int64_t off = 0;
        for (int l = 0; l < level; ++l) off += (int64_t)many_w.size() * (l == 0 ? many_R0 : many_lv[l - 1].R);
        return off + (int64_t)k * (level == 0 ? many_R0 : many_lv[level - 1].R);
    }
    // Region-major staging buffers of the (time, region) output form, one per stream that has applied
    // this plan (kept until the plan is destroyed; blocks of the scratch pool, wagg_scratch.hip).  A stream-ordered hipMallocAsync / hipFreeAsync pair
    // per apply made every call block for the whole kernel (0.28 ms enqueue against 0.01 ms without).
    struct Staging { hipStream_t stream; void *p; size_t bytes; };
    mutable std::mutex ws_mu;
    mutable std::vector<Staging> ws;
    void *staging(hipStream_t st, size_t bytes) const {
        std::lock_guard<std::mutex> lock(ws_mu);
        for (Staging &w : ws)
            if (w.stream == st) {
                if (w.bytes >= bytes) return w.p;
                if (hipStreamSynchronize(st) != hipSuccess) return nullptr;      // the old buffer may still be in use on this stream
                wagg::scratch_free(w.p);
                w.p = nullptr; w.bytes = 0;
                if (wagg::scratch_alloc(&w.p, bytes) != hipSuccess) return nullptr;
                w.bytes = bytes;
                return w.p;
            }
        void *p = nullptr;
        if (wagg::scratch_alloc(&p, bytes) != hipSuccess) return nullptr;
        ws.push_back({st, p, bytes});
        return p;
    }
    // the stream is about to be destroyed (the host pipeline's own compute stream): its staging goes with it, so the
    // list stays bounded and a later stream that happens to get the same handle starts clean
    void drop_staging(hipStream_t st) const {
        for (const wagg_plan *p : many_w) p->drop_staging(st);
        std::lock_guard<std::mutex> lock(ws_mu);
        for (size_t i = 0; i < ws.size(); ++i)
            if (ws[i].stream == st) {
                wagg::scratch_free(ws[i].p);         // (the caller has synchronised the stream)
                ws.erase(ws.begin() + (long)i);
                return;
            }
    }
    ~wagg_plan() {
        for (wagg_plan *p : many_w) delete p;
        if (timeout_host) wagg::note_cleanup(hipHostFree(timeout_host), "hipHostFree(status word)");
        // (straight back to the driver: hipFree waits for whatever the last apply on that stream left running, which a
        //  block handed to the pool's next taker would not)
        for (Staging &w : ws) wagg::scratch_free(w.p, false);
    }
};

namespace wagg {

// chunking CH_* of a plan, and the scalars of the plan the route reads (wagg_route.h)
inline const SparsePlanDev &chunking_of(const wagg_plan *plan, int ch) {
    return ch == CH_L32 ? plan->dl : ch == CH_L64 ? plan->dl64 : ch == CH_L64E ? plan->dl64e : plan->d;
}
inline RoutePlan route_plan(const wagg_plan *plan) {
    RoutePlan p;
    p.flags = plan->flags;
    p.has_lines = plan->has_lines; p.has_lines64 = plan->has_lines64; p.has_lines64e = plan->has_lines64e;
    p.G = plan->info.G; p.R = plan->info.R;
    for (int ch = 0; ch < 4; ++ch) {
        const SparsePlanDev &d = chunking_of(plan, ch);
        p.ch[ch] = {d.n_groups, d.g0_normal, d.n_part, d.n_empty, d.Gc, d.Gq};
    }
    return p;
}

template <typename T> struct PlanView {
    const int32_t *grp_chunk_begin, *grp_giant, *chunk_u_begin, *chunk_e_begin, *ucell;
    const int32_t *ent_region, *ent_seg_begin, *seg_u;
    const T *seg_w, *den, *ent_den;   // ent_den[e] = den[ent_region[e]]
    const T *seg_wx[3];          // many-plans (wagg_plan_create_many): the segment weights of weightings 1 .. NW - 1 of a pass
    const int32_t *chunk_desc;   // [n_chunks][8]: u0, nq, e0, ne, sb, ns, 0, 0
    int n_groups;
    int g0_normal;               // groups [0, g0_normal) are giant, the rest own exactly one chunk
    int c0_normal;               // first chunk of the first normal group
    // element transform applied to the data when it is loaded (tas_poly,
    // transformations.py:188: (tas - 273.15) ** power): xpow = 0 -> identity, else (x + xoff)^xpow
    T xoff;
    int xpow;
    // xpow == XF_EDD: Snyder exceedance degree days of (tasmin = X, tasmax = X2), both shifted by
    // xoff, at threshold edd_thr (transformations.py:7-93); chunk-walking kernel only
    const T *X2;
    T edd_thr[4];                // up to four thresholds per pass over the two fields
    int n_thr;
    int64_t thr_pstride;         // output of threshold k goes to out + k * thr_pstride
};

constexpr int LC_ENT = RG_MAX + 1;              // entries per chunk (loader/consumer kernels)
constexpr int LC_SEGS = SEG_MAX;                // segments per chunk the metadata block can hold

// workgroup barrier that waits for this wave's LDS traffic only: __syncthreads() also drains
// vmcnt, which would stall on the NEXT item's global loads that are deliberately in flight
__device__ __forceinline__ void lds_only_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// a chunk descriptor as the persistent kernels keep it in scalar registers
struct StreamDesc { int u0, nq, e0, ne, sb, ns; unsigned long long split; };

#ifdef WAGG_DIAG
// wagg_sparse_diag.hip (libwagg_diag.so only)
int report_lc_stamps(unsigned long long *lc_stamps, long long nw, long long n_items, hipStream_t stream);
// the MFMA-consumer loader/consumer kernel over the single-chunk groups of a plan created with WAGG_PLAN_LC_MFMA
int launch_lc_mfma(const wagg_plan *plan, const PlanView<float> &pv, const float *X, int64_t Ttot, int64_t ldx, float *kout,
                   int64_t kldo, int n_norm, bool vec, bool edd, int xpow, int nfuse, int64_t kpstride, hipStream_t stream);
#endif

}  // namespace wagg
