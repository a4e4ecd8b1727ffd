// Degree-day ladders (wagg_edd_ladder_reduce_*): out[k][p][j] = sum over the rows t of period p, in list order, on which cell j
// is in season, of snyder_edd1(X[t, j] + off, X2[t, j] + off, thr[k]) for up to WAGG_EDD_LADDER_MAX thresholds in ONE launch --
// the reference's agricultural product (validate_edd_snyder_agriculture, transformations.py:150-157: every refTemp of a
// ladder, per region and growing season).  wagg_season_reduce_* / wagg_period_reduce_* take four thresholds a call; a 41-step
// ladder costs eleven calls there, each one more pass over tasmin and tasmax.
//
// The shape is the row-list family's (wagg_rowlist.h) and the season handling is season_reduce_kernel's: a NaN term counts 0
// (S6); an in-season +-inf sets bit 0 of the status word; a value out of season is selected away and a piece none of whose
// cells is in season is not read.  With doy_dev = win_dev = NULL every listed row counts (the period sum).
// A lane cannot hold 64 x VEC fp64 sums, so the thresholds are cut into groups of EL_G and the group is one more grid dimension
// beside column block x period x part; every group reads its tasmin / tasmax pieces again (L2 serves what HBM served once).
//
// New against the four-plane kernels: snyder_edd1<float> evaluates the band expression for every value and then selects.  Here
// a wave first asks, per threshold and row, whether ANY lane has e inside the range of its in-season cells, least tasmin to
// greatest tasmax (one ballot; no cell with tasmin < e < tasmax escapes that); if none has, the
// band expression is skipped and each lane takes M - e or 0 -- the value snyder_edd1 would have selected, bit for bit, so plane
// k equals the plane wagg_season_reduce_* (or, without a season, wagg_period_reduce_* with WAGG_XF_EDD) gives for the same
// threshold when each call gets the workspace its own *_work_bytes reports.  On a 0..40 C ladder most thresholds lie outside a
// cell's diurnal range on a given day.  fp64 calls snyder_edd1<double>, the libm form the season kernel calls.
//
// EL_G = 8 thresholds a group, EL_UNROLL = 2 rows in flight.  hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage
// (VGPRs / scratch bytes / waves per SIMD; the season kernels, the no-season ones take 2-7 registers fewer; DST does not matter):
//   fp32 VEC = 4   122 / 0 / 4        fp32 VEC = 1   56 / 0 / 8        fp64 VEC = 2   119 / 0 / 4        fp64 VEC = 1   91 / 0 / 5
// No AGPRs, no LDS.  EL_UNROLL = 4 (the four-plane kernels' depth) took fp32 VEC = 4 to 136 registers = 3 waves, and holding it
// to 128 by attribute spilled 24 bytes; EL_G = 16 cannot stay under 128 at any depth (64 registers of sums alone).  From a
// handful of thresholds on the kernel is bound by arithmetic, not by its loads -- reasoning, not measurement.
#include "wagg_rowlist.h"

namespace wagg {

constexpr int EL_G = WAGG_EDD_LADDER_GROUP;
constexpr int EL_UNROLL = 2;

template <typename T> struct LadderXf {
    T off;
    int n_thr;
    T thr[WAGG_EDD_LADDER_MAX];
};

// what snyder_edd1<T> selects when NOT tmin < e < tmax, in snyder_edd1<T>'s own arithmetic (wagg_common.h): M - e where
// tasmin is not below the threshold (NaN for a NaN tasmin), else 0.  The four-plane kernels form M = sum * 0.5 and M - e in two
// instructions (M serves four thresholds there); contraction is switched off so that this does too.  (A fused sum * 0.5 - e
// would give the same bits for every sum that is not subnormal: a product with 0.5 is exact.)
template <typename T> __device__ __forceinline__ T snyder_edd1_outside(T tmin, T tmax, T e) {
#pragma clang fp contract(off)
    if constexpr (sizeof(T) == 4) {
        const T d = 0.5f * (tmax + tmin) - e;
        return !(tmin < e) ? d : T(0);
    } else {
        const T M = (tmax + tmin) / T(2);
        return !(tmin < e) ? M - e : T(0);
    }
}

// SEASON = false: doy / win are not read, every valid listed row counts.  DST = T: the finished sums go to `out`; DST = double:
// partial sums of part `s` go to `out` = the workspace (ldo = n, pstride = P * n), finished by rowlist_finish.
template <typename T, int VEC, bool SEASON, typename DST>
__global__ void __launch_bounds__(RL_BLOCK)
edd_ladder_kernel(const T *__restrict__ X, const T *__restrict__ X2, RowlistShape sh, const int32_t *__restrict__ row_begin,
                  const int32_t *__restrict__ rows, const int32_t *__restrict__ doy, const int32_t *__restrict__ win, LadderXf<T> xf,
                  DST *__restrict__ out, int64_t ldo, int64_t pstride, int32_t *__restrict__ status) {
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = (int32_t)(sg % sh.split), k0 = (int32_t)(sg / sh.split) * EL_G;
    const int kg = xf.n_thr - k0 < EL_G ? xf.n_thr - k0 : EL_G;      // thresholds of this group (>= 1 by the grid's extent)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    T thr[EL_G];                                                     // (wave-uniform: scalar registers)
#pragma unroll
    for (int k = 0; k < EL_G; ++k) thr[k] = k < kg ? xf.thr[k0 + k] : T(0);
    double acc[EL_G][VEC];
#pragma unroll
    for (int k = 0; k < EL_G; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc[k][c] = 0.0;
    bool saw_inf = false;
    if (col < sh.n) {
        int32_t w[VEC];                                              // the lane's windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (SEASON) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
            else w[c] = 0;
        }
        for (int64_t i = b; i < e; i += EL_UNROLL) {
            T x[EL_UNROLL][VEC], x2[EL_UNROLL][VEC];
            bool in[EL_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < EL_UNROLL; ++u) {
                const int64_t t = i + u < e ? (int64_t)rows[i + u] : -1;
                const bool ok = t >= 0 && t < sh.T;                  // (wave-uniform; a row index outside the field is never read)
                int32_t d = -1;
                if constexpr (SEASON) d = ok ? doy[t] : -1;          // (wave-uniform too: one scalar per row)
                bool any = false;
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    if constexpr (SEASON) in[u][c] = in_season(d, w[c]);
                    else in[u][c] = ok && col + c < sh.n;
                    any |= in[u][c];
                    x[u][c] = x2[u][c] = T(0);
                }
                if (any) {                                           // no cell of this piece in season: no load
                    load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x[u]);
                    load_piece<T, VEC>(X2 + t * sh.ldx, col, sh.n, x2[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < EL_UNROLL; ++u) {
                T lo[VEC], hi[VEC];
                // the lane's in-season cells as one range [least tasmin, greatest tasmax]: a cell whose sinusoid crosses e puts
                // e inside it, so testing the range never misses a cell (it may ask for the band expression where no single
                // cell needs it: the values are the same) and costs two compares a threshold instead of two a cell.  NaN
                // compares false: it neither widens the range nor is it in any band.
                T lane_lo = __builtin_huge_val(), lane_hi = -__builtin_huge_val();
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    lo[c] = x[u][c] + xf.off;
                    hi[c] = x2[u][c] + xf.off;
                    if (in[u][c] && lo[c] < lane_lo) lane_lo = lo[c];
                    if (in[u][c] && hi[c] > lane_hi) lane_hi = hi[c];
                }
#pragma unroll
                for (int k = 0; k < EL_G; ++k) {
                    if (k >= kg) continue;
                    const bool band = lane_lo < thr[k] && lane_hi > thr[k];      // may an in-season cell's sinusoid cross thr[k]?
                    T f[VEC];
                    if (__ballot(band) != 0ull) {                    // (wave-uniform branch)
#pragma unroll
                        for (int c = 0; c < VEC; ++c) f[c] = snyder_edd1<T>(lo[c], hi[c], thr[k]);
                    } else {                                         // no lane of the wave needs the band expression
#pragma unroll
                        for (int c = 0; c < VEC; ++c) f[c] = snyder_edd1_outside<T>(lo[c], hi[c], thr[k]);
                    }
#pragma unroll
                    for (int c = 0; c < VEC; ++c) {
                        T v = in[u][c] ? f[c] : T(0);                // selected, not multiplied: nothing out of season gets further
                        saw_inf |= __builtin_isinf(v);
                        if (v != v) v = T(0);                        // S6: a NaN term counts 0
                        acc[k][c] += (double)v;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < EL_G; ++k) {
            if (k >= kg) continue;
            DST *o = out + (int64_t)s * xf.n_thr * pstride + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
#pragma unroll
            for (int c = 0; c < VEC; ++c)
                if (col + c < sh.n) o[c] = (DST)acc[k][c];
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

template <typename T>
static int ladder_reduce(const GroupedArgs<T> &a, double offset, const double *thresholds, int n_thr) {
    static const GroupedFamily fam = {"a degree-day ladder", "tasmin_dev / tasmax_dev", 2, EL_G};
    return grouped_reduce<T>(
        fam, a, n_thr,
        [&]() -> int {
            WAGG_REQUIRE(n_thr >= 1 && n_thr <= WAGG_EDD_LADDER_MAX, "n_thr must be 1..%d, got %d", WAGG_EDD_LADDER_MAX, n_thr);
            WAGG_REQUIRE(thresholds != nullptr, "thresholds is NULL");
            return WAGG_OK;
        },
        [&](const RowlistShape &sh, bool wide, hipStream_t st) {
            LadderXf<T> xf;
            xf.off = (T)offset; xf.n_thr = n_thr;
            for (int k = 0; k < WAGG_EDD_LADDER_MAX; ++k) xf.thr[k] = (T)(k < n_thr ? thresholds[k] : 0.0);
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3 grid, auto *out, int64_t ldo, int64_t pstride) {
                using DST = std::remove_pointer_t<decltype(out)>;
                hipLaunchKernelGGL((edd_ladder_kernel<T, decltype(vec)::value, decltype(season)::value, DST>), grid, dim3(RL_BLOCK), 0, st,
                                   a.X, a.X2, sh, a.row_begin, a.rows, a.doy, a.win, xf, out, ldo, pstride, a.status);
            });
        });
}

}  // namespace wagg

extern "C" int64_t wagg_edd_ladder_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_thr) {
    return wagg::rowlist_work_bytes(n, P, n_rows, n_thr);
}

extern "C" int wagg_edd_ladder_reduce_f32(const float *tasmin_dev, const float *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                                          const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                                          const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *thresholds,
                                          int n_thr, int flags, float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev,
                                          void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::ladder_reduce<float>({tasmin_dev, tasmax_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags,
                                       out_dev, ldo, out_pstride, status_dev, work_dev, work_bytes, stream}, offset, thresholds, n_thr);
}
extern "C" int wagg_edd_ladder_reduce_f64(const double *tasmin_dev, const double *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                                          const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                                          const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *thresholds,
                                          int n_thr, int flags, double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev,
                                          void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::ladder_reduce<double>({tasmin_dev, tasmax_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags,
                                        out_dev, ldo, out_pstride, status_dev, work_dev, work_bytes, stream}, offset, thresholds, n_thr);
}
