// Spells that run across period boundaries (wagg_spell_span_*): wagg_spell_reduce_*'s three statistics with the runs NOT
// truncated at the end of a period's list -- CDD / CWD (the longest dry / wet spell, defined on spells that run through New Year),
// a December-January heat wave with min_length = 6, every month end of a period = "month" call.  wagg_spells.hip stays the
// truncating kernel, line for line; this is its sibling with another grid.
//
// THE DEFINITION.  The CHAIN is the concatenation of the periods' lists in period order: the entries
// rows[row_begin[0] : row_begin[P]], row_begin clamped as WAGG_ROWLIST_ROWS clamps it.  For cell j and threshold k:
//   HOT    entry i is hot exactly as in wagg_spell_reduce_*: t = rows[i] lies in [0, T), cell j is in season on doy[t] (when a
//          season is given) and the RAW X[t, j] passes against ceilT(thresholds[k] - offset) (>= for below = 0, < for below = 1).
//          NaN is never hot.
//   JOINS  entry i joins entry i - 1 when rows[i] == rows[i - 1] + 1 -- whether or not a period boundary, or several empty
//          periods, lie between them.  Empty lists are transparent.
//   RUN    a maximal stretch of hot, joined entries of the chain.
//   r_i    the RUNNING LENGTH at entry i: its position within its run, from 1; 0 when cold.  It is carried over boundaries.
//   l      the run's WHOLE LENGTH.
// With L = min_length, out[k][p][j] is
//   WAGG_SPELL_DAYS     the hot entries of p's list whose run has l >= L: every day is counted in its own period, whether it
//                       counts is decided by the whole run
//   WAGG_SPELL_EVENTS   the entries of p's list with r_i == L: a run counts once, in the period in which it reaches min_length
//                       (L = 1: the period in which it starts)
//   WAGG_SPELL_LONGEST  the greatest r_i over the entries of p's list, 0 for an empty list: a spell counts in a period for as
//                       long as it has lasted by then, reaching back to its start wherever that lies.  A year wholly inside one
//                       dry spell reports at least its own length; a spell from 20 December to 10 January gives 12 and 22.
//                       L must be 1.
// What follows: where no run crosses a boundary all three equal wagg_spell_reduce_* bit for bit; the sum over p of DAYS and of
// EVENTS, and the max over p of LONGEST, equal the truncating kernel's single-period result on the chain taken as one list;
// LONGEST is never below the truncating value.  Joins are found only between neighbours in the chain: with labels that pool the
// Januaries of all years nothing joins across lists and the result is wagg_spell_reduce_*'s.
//
// THE FRAME is spell_kernel's: a lane owns one 16-byte piece of a row (VEC = 1 for unaligned rows), the thresholds of a group
// are wave-uniform, the season window is read once, a piece with no cell in season is not read but still resets the runs, the
// gap test is wave-uniform, an in-season +-inf sets bit 0 of the status word, one row is in flight, STAT is a template parameter
// and `below` a wave-uniform select.  THE GRID IS THE DIFFERENCE: column block x threshold group, WITHOUT a period dimension.  A
// block walks the periods 0 .. P - 1 in order, carries run[k][c] (and the row of the entry before) across them, keeps acc[k][c]
// per period and stores out[k, p, col ..] when it leaves p's list; an empty period stores 0.  There is no per-cell state beyond
// run and acc, and the position of an entry within its period, pos = i - b_p + 1, is wave-uniform.
//
// EVENTS and LONGEST only look forward.  DAYS is the one statistic that must credit an earlier period: when r reaches L at entry
// i, L days qualify at once, min(L, pos) of them in p and the rest as the last entries of the preceding lists.  The kernel
// walks q = p - 1, p - 2, ... taking min(remaining, length of q's list) of each (the walk and what it takes are wave-uniform; it
// ends because the L joined entries exist, and at q = 0 whatever the lists say) and adds to out[k, q, col + c] by a
// read-modify-write of the value THIS LANE stored when it left q's list: one thread, one address, program order -- no atomics, no
// workspace, no second launch, and nothing read from `out` that this launch did not write.  Counts stay exact in fp32 below 2^24.
//
// THE COST.  A block walks all n_rows entries of the record, and the launch has n_colblk x groups blocks where the truncating
// kernel has P times as many: ten years of a 20 000-cell packed row (cells = "referenced") are 20 blocks of VEC = 4 lanes per
// group of thresholds, each walking 3650 rows -- far fewer than the 256 CUs.  No remedy is built (a cut of the record into
// parts would have to combine prefix / suffix / interior runs); tools/spell_span_timing.py records what it costs.
// wagg_spell_span_work_bytes is 0 and work_dev / work_bytes are ignored.
//
// hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage (VGPRs / scratch bytes / waves per SIMD), the season
// kernels (the no-season ones take 0-9 registers fewer; fp32 VEC = 4 EVENTS / LONGEST without a season: 78 = 6 waves):
//                 fp32 VEC = 4     fp32 VEC = 1     fp64 VEC = 2     fp64 VEC = 1
//   DAYS          90 / 0 / 5       30 / 0 / 7       64 / 0 / 7       33 / 0 / 7
//   EVENTS        87 / 0 / 5       28 / 0 / 8       63 / 0 / 7       30 / 0 / 7
//   LONGEST       87 / 0 / 5       28 / 0 / 8       63 / 0 / 7       30 / 0 / 7
// No scratch, no AGPRs, no LDS in any of the 24 instances -- the waves per SIMD of spell_kernel's instances.  UNLIKE
// spell_kernel, SGPRs ARE SPILLED, into VGPR lanes (v_writelane / v_readlane; they are in the VGPR counts above): the period
// loop's own scalars (P, p, b, e, the list pointers) come on top of a frame that already took 95.  EVENTS / LONGEST spill 12-20
// SGPRs in the season instances of fp32 VEC = 4 and fp64 VEC = 2 and none elsewhere, and the block of the entry loop holds no
// lane move.  The DAYS instances spill 46-99: the credit walk holds a lane mask per threshold and cell across the lists.  Its
// compares are formed behind an opaque copy of L (an empty asm), so that they are not carried out of the hot update as 32
// masks; with that the entry loop's block (523 instructions for fp32 VEC = 4) reads 14-38 spilled scalars back per entry and
// writes none.  Tried and dropped, by register count: the credit walk per threshold (107 VGPRs = 4 waves for fp32 VEC = 4) and
// a one-VGPR bit mask of the runs that reached L (116 = 4 waves: hipcc then holds the eight plane pointers across the walk).
//
// The host layer is wagg_spell.h's: wagg_spell_reduce_*'s SpellXf, its checks in its order, the pick of the STAT instance.
#include "wagg_spell.h"

namespace wagg {

constexpr int SS_G = WAGG_SPELL_GROUP;

// [b, e) = period p's list, confined to the list's extent as WAGG_ROWLIST_ROWS confines it (one part)
#define WAGG_SPAN_LIST(sh, row_begin, p, b, e)                                                \
    int64_t b = (row_begin)[p], e = (row_begin)[(p) + 1];                                     \
    b = b < 0 ? 0 : (b > (sh).n_rows ? (sh).n_rows : b);                                      \
    e = e < b ? b : (e > (sh).n_rows ? (sh).n_rows : e)

// SEASON = false: doy / win are not read, every valid listed row counts.  STAT: WAGG_SPELL_DAYS / _EVENTS / _LONGEST.
// blockIdx.x = column block + n_colblk * threshold group.
template <typename T, int VEC, bool SEASON, int STAT>
__global__ void __launch_bounds__(RL_BLOCK)
spell_span_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
                  const int32_t *__restrict__ doy, const int32_t *__restrict__ win, SpellXf<T> xf, T *out, int64_t ldo,
                  int64_t pstride, int32_t *__restrict__ status) {
    const int32_t cb = (int32_t)(blockIdx.x % (unsigned)sh.n_colblk);
    const int32_t k0 = (int32_t)(blockIdx.x / (unsigned)sh.n_colblk) * SS_G;
    const int kg = xf.n_thr - k0 < SS_G ? xf.n_thr - k0 : SS_G;      // thresholds of this group (>= 1 by the grid's extent)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    const int32_t L = xf.min_length;
    const bool below = xf.below != 0;
    T thr[SS_G];                                                     // (wave-uniform: scalar registers)
#pragma unroll
    for (int k = 0; k < SS_G; ++k) thr[k] = xf.c[k0 + k < xf.n_thr ? k0 + k : xf.n_thr - 1];      // (a ragged group repeats the last)
    int32_t run[SS_G][VEC], acc[SS_G][VEC];
#pragma unroll
    for (int k = 0; k < SS_G; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) run[k][c] = 0;
    bool saw_inf = false;
    if (col < sh.n) {
        int32_t w[VEC];                                              // the lane's windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (SEASON) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
            else w[c] = 0;
        }
        int64_t prev = -2;                                           // the row of the chain's entry before (no row follows -2)
        for (int32_t p = 0; p < sh.P; ++p) {                         // the periods in order: run and prev are carried over
            WAGG_SPAN_LIST(sh, row_begin, p, b, e);
#pragma unroll
            for (int k = 0; k < SS_G; ++k)
#pragma unroll
                for (int c = 0; c < VEC; ++c) acc[k][c] = 0;
            for (int64_t i = b; i < e; ++i) {
                const int64_t t = (int64_t)rows[i];
                const bool ok = t >= 0 && t < sh.T;                  // (wave-uniform; a row index outside the field is never read)
                const bool joins = t == prev + 1;                    // (wave-uniform: does this entry continue the one before?)
                prev = t;
                int32_t d = -1;
                if constexpr (SEASON) d = ok ? doy[t] : -1;          // (wave-uniform too: one scalar per row)
                T x[VEC];
                bool in[VEC], any = false;
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    if constexpr (SEASON) in[c] = in_season(d, w[c]);
                    else in[c] = ok && col + c < sh.n;
                    any |= in[c];
                    x[c] = T(0);
                }
                if (any) load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x);         // no cell of this piece in season: no load
                if (!joins) {                                        // behind a gap in the row numbers every run starts anew
#pragma unroll
                    for (int k = 0; k < SS_G; ++k)
#pragma unroll
                        for (int c = 0; c < VEC; ++c) run[k][c] = 0;
                }
                const int64_t pos = i - b + 1;                       // the entry's position in its period's list (wave-uniform)
                const int32_t here = pos < L ? (int32_t)pos : L;     // DAYS: the days of p that qualify when a run reaches L here
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    saw_inf |= in[c] && __builtin_isinf(x[c]);
                    const T v = in[c] ? x[c] : (T)__builtin_nan("");               // selected away: NaN is cold on either side
#pragma unroll
                    for (int k = 0; k < SS_G; ++k) {
                        const bool hot = below ? v < thr[k] : v >= thr[k];
                        const int32_t r = hot ? run[k][c] + 1 : 0;
                        run[k][c] = r;
                        if constexpr (STAT == WAGG_SPELL_DAYS) {
                            acc[k][c] += r == L ? here : (r > L ? 1 : 0);
                        } else if constexpr (STAT == WAGG_SPELL_EVENTS) {
                            acc[k][c] += r == L ? 1 : 0;
                        } else {
                            acc[k][c] = r > acc[k][c] ? r : acc[k][c];
                        }
                    }
                }
                if constexpr (STAT == WAGG_SPELL_DAYS) {
                    // the L - pos days of such a run that lie before p's list: the last entries of the lists before, newest first
                    if (pos < L) {                                   // (wave-uniform, and rare: the first L - 1 entries of a list)
                        int32_t Lq = L;                              // (opaque: the compares of this rare path are formed here, not
                        asm volatile("" : "+s"(Lq));                 //  carried out of the update above as SS_G * VEC lane masks)
                        bool reached = false;                        // did a run of this lane reach L on this entry?
#pragma unroll
                        for (int k = 0; k < SS_G; ++k)
#pragma unroll
                            for (int c = 0; c < VEC; ++c) reached |= run[k][c] == Lq;
                        int64_t rem = __ballot(reached) != 0ull ? L - pos : 0;
                        for (int32_t q = p - 1; q >= 0 && rem > 0; --q) {         // (wave-uniform, as is what it takes)
                            WAGG_SPAN_LIST(sh, row_begin, q, bq, eq);
                            const int64_t take = rem < eq - bq ? rem : eq - bq;
                            rem -= take;
                            if (take == 0) continue;                 // (an empty list: transparent)
#pragma unroll
                            for (int k = 0; k < SS_G; ++k) {
                                if (k >= kg) continue;
                                T *o = out + (int64_t)(k0 + k) * pstride + (int64_t)q * ldo + col;
#pragma unroll
                                for (int c = 0; c < VEC; ++c)        // (what this lane stored on leaving q's list, and nothing else)
                                    if (run[k][c] == Lq && col + c < sh.n) o[c] = o[c] + (T)(int32_t)take;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < SS_G; ++k) {                         // leaving p's list (an empty one: 0)
                if (k >= kg) continue;
                T *o = out + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
#pragma unroll
                for (int c = 0; c < VEC; ++c)
                    if (col + c < sh.n) o[c] = (T)acc[k][c];
            }
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

template <typename T>
static int spell_span_reduce(const GroupedArgs<T> &a, double offset, const double *thresholds, int n_thr, int min_length, int stat,
                             int below) {
    static const GroupedFamily fam = {"a spell count", "X_dev", 1, SS_G};
    return grouped_reduce<T>(
        fam, a, n_thr,                                               // (not looked at unless n_thr passes the check)
        [&]() -> int { return spell_require(n_thr, thresholds, offset, min_length, stat, below); },
        [&](const RowlistShape &got, bool wide, hipStream_t st) {
            RowlistShape sh = got;
            sh.split = 1;                                            // (no workspace went in; rowlist_finish then has nothing to add)
            const SpellXf<T> xf = spell_xf<T>(thresholds, n_thr, offset, min_length, below);
            // one block per column block and threshold group: grouped_launch's grid has the period dimension this kernel walks
            const dim3 grid((unsigned)((int64_t)sh.n_colblk * sh.aux));
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3, auto *out, int64_t ldo, int64_t pstride) {
                if constexpr (std::is_same_v<std::remove_pointer_t<decltype(out)>, T>) {      // (split = 1: never the workspace)
                    spell_with_stat<false>(stat, [&](auto stat_c) {
                        hipLaunchKernelGGL((spell_span_kernel<T, decltype(vec)::value, decltype(season)::value, decltype(stat_c)::value>),
                                           grid, dim3(RL_BLOCK), 0, st, a.X, sh, a.row_begin, a.rows, a.doy, a.win, xf, out, ldo, pstride,
                                           a.status);
                    });
                }
            });
        });
}

}  // namespace wagg

extern "C" int64_t wagg_spell_span_work_bytes(int64_t, int32_t, int64_t, int) { return 0; }

extern "C" int wagg_spell_span_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                          const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev,
                                          const int32_t *win_dev, double offset, const double *thresholds, int n_thr, int min_length,
                                          int stat, int below, int flags, float *out_dev, int64_t ldo, int64_t out_pstride,
                                          int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::spell_span_reduce<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev,
                                           ldo, out_pstride, status_dev, nullptr, 0, stream}, offset, thresholds, n_thr, min_length, stat,
                                          below);
}
extern "C" int wagg_spell_span_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                          const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev,
                                          const int32_t *win_dev, double offset, const double *thresholds, int n_thr, int min_length,
                                          int stat, int below, int flags, double *out_dev, int64_t ldo, int64_t out_pstride,
                                          int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::spell_span_reduce<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev,
                                            ldo, out_pstride, status_dev, nullptr, 0, stream}, offset, thresholds, n_thr, min_length, stat,
                                           below);
}
