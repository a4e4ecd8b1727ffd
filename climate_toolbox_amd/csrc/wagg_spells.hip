// Spell statistics (wagg_spell_reduce_*): runs of consecutive days past a threshold, per period and season, for up to
// WAGG_SPELL_MAX = 64 thresholds in ONE launch -- heat-wave / cold-spell days, the number of such events and the longest run
// (the ETCCDI / xclim spell indices; tasmax >= 35 C for >= 3 days is the usual heat wave).  The one class of temperature
// statistic the other row-list families cannot express: a day's contribution depends on its neighbours.  On the grid it is a
// (T, G) run-length scan and a masked field in front of an apply, per threshold.
//
// THE DEFINITION.  Cell j, period p, threshold k: the entries i of rows[row_begin[p] : row_begin[p + 1]] are walked IN ORDER.
// Entry i is HOT when t = rows[i] lies in [0, T), cell j is in season on doy[t] (when a season is given) and
// X[t, j] + offset >= thresholds[k] (below = 0) or < thresholds[k] (below = 1).  The comparison is the bins' exact rule
// (wagg_bins.hip): the host hands over ceilT(thresholds[k] - offset) and the kernel compares the RAW value against it, so an
// fp32 Kelvin field is classified as its exact values would be in fp64.  NaN is never hot, on either side.  A RUN is a maximal
// stretch of hot entries i, i + 1, ... with rows[i + 1] == rows[i] + 1: a gap in the row numbers (a dropped label row, another
// January of a month-of-all-years labelling), an out-of-season day, a NaN and the end of the period's list all end it.  RUNS
// ARE TRUNCATED AT PERIOD BOUNDARIES: a heat wave over New Year's Eve is two runs, one in each year.  With L = min_length:
//   WAGG_SPELL_DAYS     the hot entries that belong to runs of length >= L
//   WAGG_SPELL_EVENTS   the runs of length >= L
//   WAGG_SPELL_LONGEST  the length of the longest run (L must be 1)
// None needs a flush at the list's end: on a hot entry run += 1, on a cold one run = 0; then DAYS adds L when run == L and 1
// when run > L, EVENTS adds 1 when run == L, LONGEST takes a max.  Run and result are int32 per cell and threshold, in
// registers; the result is written in the element type (exact in fp32 up to 2^24).
//
// The shape is the row-list family's (wagg_rowlist.h) and the frame is bin_days_kernel's: a lane owns one 16-byte piece of a
// row (VEC = 1 for unaligned rows), the grid is column block x period x group, the thresholds of a group are wave-uniform
// (scalar registers), a value out of season is selected away (to NaN: it is cold, and reaches no status word), a piece none of
// whose cells is in season is not read BUT STILL RESETS THE RUNS, an in-season +-inf sets bit 0 of the status word whether it is
// hot or not.  Entries are consumed strictly in list order; the gap test (rows[i] == rows[i - 1] + 1, wave-uniform) zeroes the
// runs ahead of the entry behind a gap.  SP_UNROLL = 1: one row in flight per wave, see the registers below.
//
// THIS FAMILY NEVER SPLITS A PERIOD'S LIST.  A run does not add across parts, so wagg_spell_work_bytes is 0, the entry points
// ignore work_dev / work_bytes and hand rowlist_geometry no workspace, which makes split = 1 (spell_reduce looks at what it
// got and launches one part whatever it says).  Combining parts through (prefix run, suffix run, interior) triples is out of
// scope.  The cost: a single long period on a packed row fills fewer than RL_TARGET_BLOCKS blocks per group -- one period of a
// 20 000-cell row is 20 blocks of VEC = 4 lanes per group of thresholds.
//
// STAT is a template parameter, `below` a wave-uniform select.  The three statistics differ in the update of the result (an
// add of a two-way select, an add of a compare, a max): as a run-time switch inside the threshold loop all three updates are
// live code and the compiler holds their selects' operands across it, while a template instance carries exactly one of them.
// `below` only picks one of two compares of the same operands (x >= c / x < c; NaN fails both): a scalar select on the two
// lane masks, no register of its own, so templating it would double the instances for nothing.
// Measured with SP_UNROLL = 1, fp32 VEC = 4 / VEC = 1 / fp64 VEC = 2 / VEC = 1 season kernels, WAGG_SPELL_DAYS: the template
// 86 / 29 / 49 / 30 VGPRs, the run-time switch 88 / 36 / 52 / 36 -- the same waves per SIMD, the template never more registers.
// hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage (VGPRs / scratch bytes / waves per SIMD; the season
// kernels, the greatest of the three statistics; the no-season ones take 2-5 registers fewer):
//   fp32 VEC = 4   86 / 0 / 5        fp32 VEC = 1   29 / 0 / 8        fp64 VEC = 2   49 / 0 / 8        fp64 VEC = 1   30 / 0 / 8
// No SGPR spilled in any of the 24 instances (at most 95 SGPRs), no AGPRs, no LDS.  SP_G = WAGG_SPELL_GROUP = 8 thresholds a
// group: run and result are two int32 per threshold and cell, 64 of fp32 VEC = 4's 86 registers.  Groups of 4 took 77 (6
// waves) for twice the passes over the field.  Two rows in flight (bin_days_kernel's depth) took 131 registers = 3 waves
// with the uniform branch that zeroes the runs behind a gap, 101-116 = 4 waves with a select in its place: hipcc then holds
// both rows' compares across the run updates.  One row at 5 waves per SIMD keeps 5 loads in flight per SIMD where two rows at
// 3 waves keep 6, with 32 integer operations per cell and row to hide them behind -- reasoning, not measurement.
//
// The host layer (SpellXf and its fill, the argument checks, the pick of the STAT instance) is wagg_spell.h's, shared with the
// three sibling units.
#include "wagg_spell.h"

namespace wagg {

constexpr int SP_G = WAGG_SPELL_GROUP;
constexpr int SP_UNROLL = 1;

// SEASON = false: doy / win are not read, every valid listed row counts.  STAT: WAGG_SPELL_DAYS / _EVENTS / _LONGEST.
template <typename T, int VEC, bool SEASON, int STAT>
__global__ void __launch_bounds__(RL_BLOCK)
spell_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
             const int32_t *__restrict__ doy, const int32_t *__restrict__ win, SpellXf<T> xf, T *__restrict__ out, int64_t ldo,
             int64_t pstride, int32_t *__restrict__ status) {
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = 0, k0 = (int32_t)sg * SP_G;                     // (one part: the grid has no part dimension to speak of)
    const int kg = xf.n_thr - k0 < SP_G ? xf.n_thr - k0 : SP_G;      // thresholds of this group (>= 1 by the grid's extent)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    const int32_t L = xf.min_length;
    const bool below = xf.below != 0;
    T thr[SP_G];                                                     // (wave-uniform: scalar registers)
#pragma unroll
    for (int k = 0; k < SP_G; ++k) thr[k] = xf.c[k0 + k < xf.n_thr ? k0 + k : xf.n_thr - 1];      // (a ragged group repeats the last)
    int32_t run[SP_G][VEC], acc[SP_G][VEC];
#pragma unroll
    for (int k = 0; k < SP_G; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) run[k][c] = acc[k][c] = 0;
    bool saw_inf = false;
    if (col < sh.n) {
        int32_t w[VEC];                                              // the lane's windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (SEASON) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
            else w[c] = 0;
        }
        int64_t prev = -2;                                           // the row of the entry before (no row follows -2)
        for (int64_t i = b; i < e; i += SP_UNROLL) {
            T x[SP_UNROLL][VEC];
            bool in[SP_UNROLL][VEC], joins[SP_UNROLL];
#pragma unroll
            for (int u = 0; u < SP_UNROLL; ++u) {
                const int64_t t = i + u < e ? (int64_t)rows[i + u] : -1;
                const bool ok = t >= 0 && t < sh.T;                  // (wave-uniform; a row index outside the field is never read)
                joins[u] = t == prev + 1;                            // (wave-uniform: does this entry continue the one before?)
                prev = t;
                int32_t d = -1;
                if constexpr (SEASON) d = ok ? doy[t] : -1;          // (wave-uniform too: one scalar per row)
                bool any = false;
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    if constexpr (SEASON) in[u][c] = in_season(d, w[c]);
                    else in[u][c] = ok && col + c < sh.n;
                    any |= in[u][c];
                    x[u][c] = T(0);
                }
                if (any) load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x[u]);      // no cell of this piece in season: no load
            }
#pragma unroll
            for (int u = 0; u < SP_UNROLL; ++u) {                    // strictly in list order
                if (!joins[u]) {                                     // behind a gap in the row numbers every run starts anew
#pragma unroll
                    for (int k = 0; k < SP_G; ++k)
#pragma unroll
                        for (int c = 0; c < VEC; ++c) run[k][c] = 0;
                }
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    saw_inf |= in[u][c] && __builtin_isinf(x[u][c]);
                    const T v = in[u][c] ? x[u][c] : (T)__builtin_nan("");       // selected away: NaN is cold on either side
#pragma unroll
                    for (int k = 0; k < SP_G; ++k) {
                        const bool hot = below ? v < thr[k] : v >= thr[k];
                        const int32_t r = hot ? run[k][c] + 1 : 0;
                        run[k][c] = r;
                        if constexpr (STAT == WAGG_SPELL_DAYS) acc[k][c] += r == L ? L : (r > L ? 1 : 0);
                        else if constexpr (STAT == WAGG_SPELL_EVENTS) acc[k][c] += r == L ? 1 : 0;
                        else acc[k][c] = r > acc[k][c] ? r : acc[k][c];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < SP_G; ++k) {
            if (k >= kg) continue;
            T *o = out + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
#pragma unroll
            for (int c = 0; c < VEC; ++c)
                if (col + c < sh.n) o[c] = (T)acc[k][c];
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

template <typename T>
static int spell_reduce(const GroupedArgs<T> &a, double offset, const double *thresholds, int n_thr, int min_length, int stat, int below) {
    static const GroupedFamily fam = {"a spell count", "X_dev", 1, SP_G};
    return grouped_reduce<T>(
        fam, a, n_thr,                                               // (not looked at unless n_thr passes the check)
        [&]() -> int { return spell_require(n_thr, thresholds, offset, min_length, stat, below); },
        [&](const RowlistShape &got, bool wide, hipStream_t st) {
            RowlistShape sh = got;
            sh.split = 1;                                            // (no workspace went in: rowlist_geometry cannot cut a list; a run
            const SpellXf<T> xf = spell_xf<T>(thresholds, n_thr, offset, min_length, below);      // does not add across parts)
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3 grid, auto *out, int64_t ldo, int64_t pstride) {
                if constexpr (std::is_same_v<std::remove_pointer_t<decltype(out)>, T>) {      // (split = 1: never the workspace)
                    spell_with_stat<false>(stat, [&](auto stat_c) {
                        hipLaunchKernelGGL((spell_kernel<T, decltype(vec)::value, decltype(season)::value, decltype(stat_c)::value>), grid,
                                           dim3(RL_BLOCK), 0, st, a.X, sh, a.row_begin, a.rows, a.doy, a.win, xf, out, ldo, pstride,
                                           a.status);
                    });
                }
            });
        });
}

}  // namespace wagg

extern "C" int64_t wagg_spell_work_bytes(int64_t, int32_t, int64_t, int) { return 0; }

extern "C" int wagg_spell_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                     const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                     double offset, const double *thresholds, int n_thr, int min_length, int stat, int below, int flags,
                                     float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::spell_reduce<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                      out_pstride, status_dev, nullptr, 0, stream}, offset, thresholds, n_thr, min_length, stat, below);
}
extern "C" int wagg_spell_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                     const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                     double offset, const double *thresholds, int n_thr, int min_length, int stat, int below, int flags,
                                     double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::spell_reduce<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                       out_pstride, status_dev, nullptr, 0, stream}, offset, thresholds, n_thr, min_length, stat, below);
}
