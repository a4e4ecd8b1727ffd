// Growing-season totals (wagg_season_reduce_*): out[k][p][j] = sum over the rows t of period p, in list order, on which cell
// j is in season, of f_k(X[t, j]) -- the period sum of wagg_period.hip with one more predicate per cell: a packed day-of-year
// window (include/wagg.h: bits 0-9 first day, 10-19 last day, 20 invert, 21 null), tested against the row's day of year.
// The sum runs in FRONT of the aggregation only (climate_toolbox_amd/seasons.py): the masked daily result is linear in the
// field, weights and denominators do not depend on time, a day out of season counts 0 like a NaN term (S6).
//
// The shape is the row-list family's (wagg_rowlist.h); day-of-year bookkeeping is wave-uniform like the row's.  Particular to
// this kernel: the lane reads its cells' windows once, issues NO load for a row on which none of its cells is in season
// (seasons are spatially coherent: whole lines drop out) and SELECTS an out-of-season value away instead of multiplying it by
// zero -- NaN or +-inf out of season reaches neither a sum nor the status word.  With every window open all year the
// arithmetic is that of wagg_period_reduce_*, bit for bit.  wagg_season_mask materialises the mask itself (0 / 1 / NaN), the
// reference's (lat, lon, time) array.
#include "wagg_rowlist.h"

namespace wagg {

constexpr int SR_UNROLL = 4;

// DST = T: the finished sums go to `out`; DST = double: partial sums of part `s` go to `out` = the workspace (ldo = n,
// pstride = P * n), finished by rowlist_finish.
template <typename T, int VEC, int MODE, typename DST>
__global__ void __launch_bounds__(RL_BLOCK)
season_reduce_kernel(const T *__restrict__ X, const T *__restrict__ X2, RowlistShape sh, const int32_t *__restrict__ row_begin,
                     const int32_t *__restrict__ rows, const int32_t *__restrict__ doy, const int32_t *__restrict__ win,
                     RowlistXf<T> xf, DST *__restrict__ out, int64_t ldo, int64_t pstride, int32_t *__restrict__ status) {
    constexpr int NPL = MODE == RL_NONE ? 1 : RL_MAX_PLANES;
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = (int32_t)sg;
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    double acc[NPL][VEC];
#pragma unroll
    for (int k = 0; k < NPL; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc[k][c] = 0.0;
    bool saw_inf = false;
    if (col < sh.n) {
        int32_t w[VEC];                                          // the lane's windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
        for (int64_t i = b; i < e; i += SR_UNROLL) {
            T x[SR_UNROLL][VEC], x2[SR_UNROLL][VEC];
            bool in[SR_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < SR_UNROLL; ++u) {
                const int64_t t = i + u < e ? (int64_t)rows[i + u] : -1;
                const bool ok = t >= 0 && t < sh.T;              // (wave-uniform; a row index outside the field is never read)
                const int32_t d = ok ? doy[t] : -1;              // (wave-uniform too: one scalar per row)
                bool any = false;
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    in[u][c] = in_season(d, w[c]);
                    any |= in[u][c];
                    x[u][c] = x2[u][c] = T(0);
                }
                if (any) {                                       // no cell of this piece in season: no load
                    load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x[u]);
                    if constexpr (MODE == RL_EDD) load_piece<T, VEC>(X2 + t * sh.ldx, col, sh.n, x2[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < SR_UNROLL; ++u) {
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    T f[NPL];
                    if constexpr (MODE == RL_NONE) {
                        f[0] = x[u][c];
                    } else if constexpr (MODE == RL_POLY) {
                        // xform1's own multiplication chain, continued: f[k] is bit for bit xform1(x, off, pow_first + k)
                        const T y = x[u][c] + xf.off;
                        f[0] = xform1<T>(x[u][c], xf.off, xf.pow_first);
#pragma unroll
                        for (int k = 1; k < NPL; ++k) f[k] = f[k - 1] * y;
                    } else {
                        const T lo = x[u][c] + xf.off, hi = x2[u][c] + xf.off;
#pragma unroll
                        for (int k = 0; k < NPL; ++k) f[k] = k < xf.planes ? snyder_edd1<T>(lo, hi, xf.thr[k]) : T(0);
                    }
#pragma unroll
                    for (int k = 0; k < NPL; ++k) {
                        if (k >= xf.planes) continue;
                        T v = in[u][c] ? f[k] : T(0);            // selected, not multiplied: nothing out of season gets further
                        saw_inf |= __builtin_isinf(v);
                        if (v != v) v = T(0);                    // S6: a NaN term counts 0
                        acc[k][c] += (double)v;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            if (k >= xf.planes) continue;
            DST *o = out + (int64_t)s * xf.planes * pstride + (int64_t)k * pstride + (int64_t)p * ldo + col;
#pragma unroll
            for (int c = 0; c < VEC; ++c)
                if (col + c < sh.n) o[c] = (DST)acc[k][c];
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

// out[j][t] = NaN for a null window, else 1 / 0 as cell j is in season on day doy[t]
__global__ void season_mask_kernel(const int32_t *__restrict__ doy, int64_t T, const int32_t *__restrict__ win, int64_t n,
                                   double *__restrict__ out) {
    const int64_t total = n * T, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int32_t w = win[i / T], d = doy[i % T];
        out[i] = (w & RL_WIN_NULL) ? __builtin_nan("") : (in_season(d, w) ? 1.0 : 0.0);
    }
}

template <typename T, int VEC, int MODE>
static void launch_season(const T *X, const T *X2, const RowlistShape &sh, const int32_t *row_begin, const int32_t *rows,
                          const int32_t *doy, const int32_t *win, const RowlistXf<T> &xf, T *out, int64_t ldo, int64_t pstride,
                          double *work, int32_t *status, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)sh.n_colblk * sh.P * sh.split)), block(RL_BLOCK);
    if (sh.split > 1)
        hipLaunchKernelGGL((season_reduce_kernel<T, VEC, MODE, double>), grid, block, 0, st, X, X2, sh, row_begin, rows, doy, win, xf, work,
                           sh.n, (int64_t)sh.P * sh.n, status);
    else
        hipLaunchKernelGGL((season_reduce_kernel<T, VEC, MODE, T>), grid, block, 0, st, X, X2, sh, row_begin, rows, doy, win, xf, out, ldo,
                           pstride, status);
}

template <typename T>
static int season_reduce(const T *X, const T *X2, int64_t Ttot, int64_t n, int64_t ldx, const int32_t *row_begin, const int32_t *rows,
                         int32_t P, int64_t n_rows, const int32_t *doy, const int32_t *win, int transform, double offset, int pow_first,
                         int n_pow, const double *thresholds, int n_thr, int flags, T *out, int64_t ldo, int64_t pstride, int32_t *status,
                         void *work, int64_t work_bytes, void *stream) {
    clear_error();
    WAGG_TRY(rowlist_require_sizes(Ttot, n, P, n_rows));
    WAGG_REQUIRE(transform == WAGG_XF_NONE || transform == WAGG_XF_POLY || transform == WAGG_XF_EDD, "unknown transform %d", transform);
    WAGG_REQUIRE((flags & ~WAGG_PERIOD_ROWS_CHECKED) == 0, "unknown flags 0x%x (a season total has no keep-NaN form)", flags);
    RowlistXf<T> xf;
    WAGG_TRY(rowlist_xf<T>(transform, offset, pow_first, n_pow, thresholds, n_thr, xf));
    WAGG_TRY(rowlist_require_layout(n, ldx, ldo, P, xf.planes, pstride, work, work_bytes, status, row_begin, rows, n_rows));
    WAGG_REQUIRE(Ttot == 0 || doy != nullptr, "NULL pointer (doy_dev)");
    WAGG_REQUIRE(n == 0 || win != nullptr, "NULL pointer (win_dev)");
    if (P == 0 || n == 0) return WAGG_OK;
    WAGG_REQUIRE(out != nullptr, "NULL pointer (out_dev)");
    WAGG_REQUIRE(n_rows == 0 || Ttot == 0 || (X != nullptr && (transform != WAGG_XF_EDD || X2 != nullptr)), "NULL pointer (X_dev / X2_dev)");
    hipStream_t st = (hipStream_t)stream;
    WAGG_TRY(rowlist_check_rows(row_begin, P, rows, n_rows, Ttot, flags, st));
    RowlistShape sh;
    sh.T = Ttot; sh.n = n; sh.ldx = ldx; sh.n_rows = n_rows; sh.P = P; sh.aux = 0;
    bool wide;
    WAGG_REQUIRE(rowlist_geometry(sh, wide, (int)sizeof(T), X, transform == WAGG_XF_EDD ? X2 : nullptr, xf.planes, work, work_bytes),
                 "too many pieces x periods for one launch");
    constexpr int V = 16 / (int)sizeof(T);
    double *w = static_cast<double *>(work);
#define WAGG_SR_LAUNCH(VEC, MODE) launch_season<T, VEC, MODE>(X, X2, sh, row_begin, rows, doy, win, xf, out, ldo, pstride, w, status, st)
    if (wide) {
        if (transform == WAGG_XF_NONE) WAGG_SR_LAUNCH(V, RL_NONE);
        else if (transform == WAGG_XF_POLY) WAGG_SR_LAUNCH(V, RL_POLY);
        else WAGG_SR_LAUNCH(V, RL_EDD);
    } else {
        if (transform == WAGG_XF_NONE) WAGG_SR_LAUNCH(1, RL_NONE);
        else if (transform == WAGG_XF_POLY) WAGG_SR_LAUNCH(1, RL_POLY);
        else WAGG_SR_LAUNCH(1, RL_EDD);
    }
#undef WAGG_SR_LAUNCH
    WAGG_HIP(hipGetLastError());
    return rowlist_finish<T>(w, sh.split, xf.planes, P, n, out, ldo, pstride, st);
}

}  // namespace wagg

extern "C" int64_t wagg_season_reduce_work_bytes(int64_t n, int32_t P, int64_t n_rows, int planes) {
    return wagg::rowlist_work_bytes(n, P, n_rows, planes);
}

extern "C" int wagg_season_reduce_f32(const float *X_dev, const float *X2_dev, int64_t T, int64_t n, int64_t ldx,
                                      const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                                      const int32_t *doy_dev, const int32_t *win_dev, int transform, double offset, int pow_first,
                                      int n_pow, const double *thresholds, int n_thr, int flags, float *out_dev, int64_t ldo,
                                      int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::season_reduce<float>(X_dev, X2_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, transform, offset,
                                      pow_first, n_pow, thresholds, n_thr, flags, out_dev, ldo, out_pstride, status_dev, work_dev, work_bytes,
                                      stream);
}
extern "C" int wagg_season_reduce_f64(const double *X_dev, const double *X2_dev, int64_t T, int64_t n, int64_t ldx,
                                      const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                                      const int32_t *doy_dev, const int32_t *win_dev, int transform, double offset, int pow_first,
                                      int n_pow, const double *thresholds, int n_thr, int flags, double *out_dev, int64_t ldo,
                                      int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::season_reduce<double>(X_dev, X2_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, transform, offset,
                                       pow_first, n_pow, thresholds, n_thr, flags, out_dev, ldo, out_pstride, status_dev, work_dev,
                                       work_bytes, stream);
}

extern "C" int wagg_season_mask(const int32_t *doy_dev, int64_t T, const int32_t *win_dev, int64_t n, double *out_dev, void *stream) {
    wagg::clear_error();
    WAGG_REQUIRE(T >= 0 && n >= 0, "negative size (T=%lld, n=%lld)", (long long)T, (long long)n);
    if (T == 0 || n == 0) return WAGG_OK;
    WAGG_REQUIRE(doy_dev != nullptr && win_dev != nullptr && out_dev != nullptr, "NULL pointer (doy_dev / win_dev / out_dev)");
    const int64_t nb = (n * T + 255) / 256;
    hipLaunchKernelGGL(wagg::season_mask_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream, doy_dev, T,
                       win_dev, n, out_dev);
    WAGG_HIP(hipGetLastError());
    return WAGG_OK;
}
