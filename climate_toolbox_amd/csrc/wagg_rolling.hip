// Rolling-window extremes (wagg_rolling_reduce_*): the greatest or least running sum (or mean) over W consecutive days, per period
// and season, for up to WAGG_ROLL_MAX_WINDOWS = 8 window lengths W = 1 .. WAGG_ROLL_WINDOW_MAX = 16 in ONE launch -- TXx / TNn
// (W = 1), the hottest or coldest N-day mean, Rx1day / Rx5day (sums of precipitation).  The second row-list family in which a
// day's contribution depends on its neighbours (after wagg_spells.hip) and the first whose period reduction is a float extreme,
// not a sum.  On the grid it is a (T, G) rolling mean and an amax per period, per window length.
//
// THE DEFINITION.  Cell j, period p, window length W: the entries i of rows[row_begin[p] : row_begin[p + 1]] are walked IN ORDER,
// as wagg_spells.hip walks them.  Entry i is VALID when t = rows[i] lies in [0, T), cell j is in season on doy[t] (when a season
// is given) and X[t, j] is not NaN.  A WINDOW of length W ends at entry i when the entries i - W + 1 .. i all lie in this period's
// list, their row numbers ascend by one and all are valid: a gap in the row numbers, an out-of-season day, a NaN and the start of
// the list invalidate every window that would hold them.  WINDOWS NEVER REACH ACROSS A PERIOD BOUNDARY: a 5-day window ending on
// 2 January does not exist in the new year (as the spells' runs are truncated there).  The window's sum is formed in fp64,
// NEWEST TO OLDEST,  s_W = ((x[i] + x[i-1]) + x[i-2]) + ... + x[i-W+1],  each x the raw element as a double (no Kelvin shift on
// single values).  The partial sums of that one chain are the sums of EVERY shorter window ending at i, so Wmax - 1 additions per
// cell and day serve all windows of a launch; the chain holds no product, so nothing can be contracted into an fma and a NumPy
// restatement gives the same bits (tests/rolling_ref.py).  WAGG_ROLL_MAX: m = -inf, then m = s > m ? s : m over the windows in
// list order; WAGG_ROLL_MIN: +inf and <.  The result is rounded ONCE from fp64 to the element type: WAGG_ROLL_MEAN
// m / (double)W + offset, WAGG_ROLL_SUM m + woff[k] with woff[k] = (double)W_k * offset formed on the host.  Division by W is
// monotone: the extreme of the sums, divided once, is the extreme of the means.  A period without a valid window for a cell
// (an empty list, one shorter than W, all gaps / out of season / NaN) gives NaN.  An in-season +-inf sets bit 0 of the status word.
//
// The shape is the row-list family's (wagg_rowlist.h), the frame spell_kernel's: a lane owns one 16-byte piece of a row (VEC = 1
// for unaligned rows), the grid is column block x period (x one group: WAGG_ROLL_GROUP = WAGG_ROLL_MAX_WINDOWS, the field is read
// once a launch), a piece none of whose cells is in season is not read BUT STILL INVALIDATES THE WINDOWS, the gap test is
// wave-uniform.  THE SLIDING WINDOW LIVES IN REGISTERS: the day loop is unrolled by the ring length RING (4, 8 or 16, the smallest
// that holds the launch's longest window), so every ring slot has a static index (a dynamically indexed array would go to scratch;
// the unrolling is spelled as RING calls of one always-inlined step, because hipcc declines `#pragma unroll` on a body this size).
// Step u stores its day in slot u and adds the chain over slots u - 1, u - 2, ... (mod RING).  THE EXTREMES ARE KEPT PER CHAIN
// LENGTH, m[len - 1] for len = 1 .. RING, not per window of the call: the chain passes every length on its way to the longest, and
// an extreme per requested window would need, at every length, a branch per window of the call (8 x 16 guarded updates a step:
// that form, tried first, spilled 30-360 SGPRs, took up to 202 VGPRs and 25 000 lines of ISA an instance, and left RING = 16 rolled).
// So a length takes its sum where the cell's valid-run counter (int32: + 1 on a valid entry, 0 on an invalid one and behind a gap)
// has reached it, behind ONE wave-uniform test of the bit `need >> len & 1` (is any window of the call len days long?), and the
// planes are picked from m[] when the list is through (windows[k] == len, wave-uniform, once a block).  Duplicate windows cost
// nothing.  Stale and NaN slots are harmless: they only enter sums of lengths the counter rules out.  The greatest run of a list
// says whether a window of length W existed at all (NaN otherwise): one more int32 per cell, no flag per window.  The steps
// past the end of a list are invalid entries.
//
// THIS FAMILY NEVER SPLITS A PERIOD'S LIST (a window does not add across parts): wagg_rolling_work_bytes is 0, the entry points
// ignore work_dev / work_bytes, which makes split = 1, as spell_reduce does.
//
// STAT (max / min) is a template parameter.  Measured against a wave-uniform run-time select of the two compares (and of the
// starting value), season kernels, VGPRs / scratch bytes: fp32 VEC = 4 RING 4 / 8: template 117 / 0 and 214 / 0, select 91 / 176
// and 156 / 304; fp64 VEC = 2: template 58 / 0 and 99 / 0, select 72 / 96 and 71 / 160; the VEC = 1 instances within 4 registers
// of each other, no scratch either way.  The select sends every 16-byte instance to scratch; the template doubles the instances.
// hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage (VGPRs / scratch bytes / waves per SIMD; the season
// kernels; max and min take the same):
//   fp32 VEC = 4   RING 4  117 / 0 / 4    RING 8  214 / 0 / 2    (RING 16: not built, below)
//   fp32 VEC = 1   RING 4   37 / 0 / 8    RING 8   63 / 0 / 8    RING 16  110 / 0 / 4
//   fp64 VEC = 2   RING 4   58 / 0 / 8    RING 8   99 / 0 / 4    (RING 16: not built, below)
//   fp64 VEC = 1   RING 4   33 / 0 / 8    RING 8   55 / 0 / 8    RING 16   94 / 0 / 5
// The no-season kernels take 0-6 registers fewer.  No scratch, no AGPRs, no LDS in any of the 40 instances.  hipcc keeps more
// than the state (RING elements and RING doubles per cell, two int32) in registers: it issues the loads of several steps ahead
// of their chains, and it spills SGPRs into VGPR lanes (none in the RING 4 VEC = 1 kernels, up to 80 in fp32 VEC = 4 RING 8, 60 in
// the RING 16 kernels) -- lanes, not memory.  RING = 16 ALWAYS RUNS ON VEC = 1, aligned rows included: the 16-byte instances took
// 256 VGPRs + 162 AGPRs (fp32 VEC = 4, 1 wave per SIMD) and 180 VGPRs (fp64 VEC = 2, 2 waves) against 110 / 94 registers and
// 4 / 5 waves for one cell per lane, whose 4- and 8-byte loads of consecutive lanes still coalesce; the host routes windows above
// 8 days there and those two instances are not built.  That VEC = 1 at 4-5 waves is the faster of the two for RING = 16 is
// reasoning from these numbers, not a measurement; fp32 VEC = 4 at RING 8 (2 waves, 4 cells a lane) against VEC = 1 (8 waves)
// has not been measured either and stays on the 16-byte loads of the other families.
#include "wagg_rowlist.h"

#include <cmath>
#include <utility>

namespace wagg {

constexpr int RO_G = WAGG_ROLL_GROUP;
static_assert(WAGG_ROLL_MAX_WINDOWS <= RO_G, "one group serves a launch: the field is read once");

struct RollXf {
    int n_win, wmax, of;
    uint32_t need;                              // bit len is set when a window of the call is len days long
    int w[RO_G];                                // the window lengths, in the caller's order
    double offset, woff[RO_G];                  // woff[k] = (double)w[k] * offset
};

template <typename F, int... U> __device__ __forceinline__ void for_each_slot(F &&f, std::integer_sequence<int, U...>) {
    (f(std::integral_constant<int, U>{}), ...);
}

// SEASON = false: doy / win are not read, every listed row counts.  RING >= xf.wmax.  STAT: WAGG_ROLL_MAX / WAGG_ROLL_MIN.
template <typename T, int VEC, bool SEASON, int RING, int STAT>
__global__ void __launch_bounds__(RL_BLOCK)
rolling_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
               const int32_t *__restrict__ doy, const int32_t *__restrict__ win, RollXf xf, T *__restrict__ out, int64_t ldo,
               int64_t pstride, int32_t *__restrict__ status) {
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = 0;                                             // (one part, one group: sg is 0)
    (void)sg;
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    const int wmax = xf.wmax;
    const uint32_t need = xf.need;
    T ring[RING][VEC];
    double m[RING][VEC];                                             // m[len - 1]: the extreme of the windows of len days
    int32_t run[VEC], longest[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
        run[c] = longest[c] = 0;
#pragma unroll
        for (int u = 0; u < RING; ++u) {
            ring[u][c] = T(0);
            m[u][c] = STAT == WAGG_ROLL_MAX ? -HUGE_VAL : HUGE_VAL;
        }
    }
    bool saw_inf = false;
    if (col < sh.n) {
        int32_t w[VEC];                                              // the lane's season windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (SEASON) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
            else w[c] = 0;
        }
        int64_t prev = -2;                                           // the row of the entry before (no row follows -2)
        for (int64_t i = b; i < e; i += RING) {
            auto step = [&](auto slot) __attribute__((always_inline)) {        // strictly in list order; slot u is static
                constexpr int u = decltype(slot)::value;
                const int64_t t = i + u < e ? (int64_t)rows[i + u] : -1;      // (past the list's end: an invalid entry)
                const bool ok = t >= 0 && t < sh.T;                  // (wave-uniform; a row index outside the field is never read)
                const bool joins = t == prev + 1;                    // (wave-uniform: does this entry continue the one before?)
                prev = t;
                int32_t d = -1;
                if constexpr (SEASON) d = ok ? doy[t] : -1;          // (wave-uniform too: one scalar per row)
                bool in[VEC], any = false;
                T x[VEC];
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    if constexpr (SEASON) in[c] = in_season(d, w[c]);
                    else in[c] = ok && col + c < sh.n;
                    any |= in[c];
                    x[c] = T(0);
                }
                if (any) load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x);        // no cell of this piece in season: no load
                double sum[VEC];
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    saw_inf |= in[c] && __builtin_isinf(x[c]);
                    const bool valid = in[c] && x[c] == x[c];
                    run[c] = valid ? (joins ? run[c] + 1 : 1) : 0;   // behind a gap in the row numbers every window starts anew
                    longest[c] = run[c] > longest[c] ? run[c] : longest[c];
                    ring[u][c] = x[c];
                    sum[c] = (double)x[c];
                }
#pragma unroll
                for (int len = 1; len <= RING; ++len) {              // the chain, newest to oldest: sum = s_len
                    if (len <= wmax) {                               // (wave-uniform)
                        if (len > 1) {
#pragma unroll
                            for (int c = 0; c < VEC; ++c) sum[c] += (double)ring[(u + RING - (len - 1)) % RING][c];
                        }
                        if ((need >> len & 1u) != 0u) {              // (wave-uniform: a window of the call is len days long)
#pragma unroll
                            for (int c = 0; c < VEC; ++c) {
                                const bool take = run[c] >= len && (STAT == WAGG_ROLL_MAX ? sum[c] > m[len - 1][c] : sum[c] < m[len - 1][c]);
                                m[len - 1][c] = take ? sum[c] : m[len - 1][c];
                            }
                        }
                    }
                }
            };
            for_each_slot(step, std::make_integer_sequence<int, RING>{});
        }
        for (int k = 0; k < xf.n_win; ++k) {                          // plane k is the window of windows[k] days
            const int32_t W = xf.w[k];
            const double woff = xf.woff[k];
            T *o = out + (int64_t)k * pstride + (int64_t)p * ldo + col;
#pragma unroll
            for (int len = 1; len <= RING; ++len) {
                if (W != len) continue;                              // (wave-uniform: m[] is never indexed by a run-time value)
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    const double r = xf.of == WAGG_ROLL_MEAN ? m[len - 1][c] / (double)len + xf.offset : m[len - 1][c] + woff;
                    if (col + c < sh.n) o[c] = longest[c] >= len ? (T)r : (T)__builtin_nan("");     // no valid window: no value
                }
            }
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

template <typename T>
static int rolling_reduce(const GroupedArgs<T> &a, double offset, const int32_t *windows, int n_win, int stat, int of) {
    static const GroupedFamily fam = {"a rolling extreme", "X_dev", 1, RO_G};
    return grouped_reduce<T>(
        fam, a, n_win,                                               // (not looked at unless n_win passes the check)
        [&]() -> int {
            WAGG_REQUIRE(n_win >= 1 && n_win <= WAGG_ROLL_MAX_WINDOWS, "n_win must be 1..%d, got %d", WAGG_ROLL_MAX_WINDOWS, n_win);
            WAGG_REQUIRE(windows != nullptr, "windows is NULL");
            for (int k = 0; k < n_win; ++k)
                WAGG_REQUIRE(windows[k] >= 1 && windows[k] <= WAGG_ROLL_WINDOW_MAX, "window %d must be 1..%d days, got %d", k,
                             WAGG_ROLL_WINDOW_MAX, (int)windows[k]);
            WAGG_REQUIRE(std::isfinite(offset), "offset must be finite");
            WAGG_REQUIRE(stat == WAGG_ROLL_MAX || stat == WAGG_ROLL_MIN, "stat must be WAGG_ROLL_MAX or WAGG_ROLL_MIN, got %d", stat);
            WAGG_REQUIRE(of == WAGG_ROLL_MEAN || of == WAGG_ROLL_SUM, "of must be WAGG_ROLL_MEAN or WAGG_ROLL_SUM, got %d", of);
            WAGG_REQUIRE((a.n + RL_BLOCK - 1) / RL_BLOCK * (int64_t)a.P < (int64_t)0x7fffffff,      // (RING = 16 runs one cell a lane)
                         "too many pieces x periods for one launch");
            return WAGG_OK;
        },
        [&](const RowlistShape &got, bool wide, hipStream_t st) {
            RowlistShape sh = got;
            if (sh.split != 1) sh.split = 1;                         // (no workspace went in; a window does not add across parts)
            RollXf xf = {};
            xf.n_win = n_win;
            xf.of = of;
            xf.offset = offset;
            for (int k = 0; k < n_win; ++k) {
                xf.w[k] = windows[k];
                xf.woff[k] = (double)windows[k] * offset;
                xf.need |= 1u << windows[k];
                xf.wmax = windows[k] > xf.wmax ? windows[k] : xf.wmax;
            }
            // RING = 16 runs on VEC = 1 whatever the alignment (the registers of the 16-byte instances: header), so those are not built
            if (wide && xf.wmax > 8) {
                wide = false;
                sh.n_colblk = (int32_t)((sh.n + RL_BLOCK - 1) / RL_BLOCK);
            }
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3 grid, auto *out, int64_t ldo, int64_t pstride) {
                if constexpr (std::is_same_v<std::remove_pointer_t<decltype(out)>, T>) {      // (split = 1: never the workspace)
                    auto go = [&](auto ring_c, auto stat_c) {
                        hipLaunchKernelGGL((rolling_kernel<T, decltype(vec)::value, decltype(season)::value, decltype(ring_c)::value,
                                                           decltype(stat_c)::value>),
                                           grid, dim3(RL_BLOCK), 0, st, a.X, sh, a.row_begin, a.rows, a.doy, a.win, xf, out, ldo, pstride,
                                           a.status);
                    };
                    auto with_stat = [&](auto ring_c) {
                        if (stat == WAGG_ROLL_MAX) go(ring_c, std::integral_constant<int, WAGG_ROLL_MAX>{});
                        else go(ring_c, std::integral_constant<int, WAGG_ROLL_MIN>{});
                    };
                    if (xf.wmax <= 4) with_stat(std::integral_constant<int, 4>{});            // the smallest ring that holds wmax
                    else if (xf.wmax <= 8) with_stat(std::integral_constant<int, 8>{});
                    else if constexpr (decltype(vec)::value == 1) with_stat(std::integral_constant<int, 16>{});
                }
            });
        });
}

}  // namespace wagg

extern "C" int64_t wagg_rolling_work_bytes(int64_t, int32_t, int64_t, int) { return 0; }

extern "C" int wagg_rolling_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                       const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                       double offset, const int32_t *windows, int n_win, int stat, int of, int flags, float *out_dev,
                                       int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::rolling_reduce<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                        out_pstride, status_dev, nullptr, 0, stream}, offset, windows, n_win, stat, of);
}
extern "C" int wagg_rolling_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                       const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                       double offset, const int32_t *windows, int n_win, int stat, int of, int flags, double *out_dev,
                                       int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::rolling_reduce<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                         out_pstride, status_dev, nullptr, 0, stream}, offset, windows, n_win, stat, of);
}
