// Growing-season totals (wagg_season_reduce_*): out[k][p][j] = sum over the rows t of period p, in list order, on which cell
// j is in season, of f_k(X[t, j]) -- the period sum of wagg_period.hip with one more predicate per cell: a packed day-of-year
// window (include/wagg.h: bits 0-9 first day, 10-19 last day, 20 invert, 21 null), tested against the row's day of year.
// The sum runs in FRONT of the aggregation only (climate_toolbox_amd/seasons.py): the masked daily result is linear in the
// field, weights and denominators do not depend on time, a day out of season counts 0 like a NaN term (S6).
//
// Same shape as period_reduce_kernel: a lane owns one 16-byte piece of a row and walks its period's row list with SR_UNROLL
// loads in flight; period, row and day-of-year bookkeeping is wave-uniform; fp64 accumulation rounded once; short grids cut
// the lists into parts that a second launch adds in part order; no atomics on a sum.  New: the lane reads its cells' windows
// once, issues NO load for a row on which none of its cells is in season (seasons are spatially coherent: whole lines drop
// out) and SELECTS an out-of-season value away instead of multiplying it by zero -- NaN or +-inf out of season reaches
// neither a sum nor the status word.  With every window open all year the arithmetic is that of wagg_period_reduce_*, bit
// for bit.  wagg_season_mask materialises the mask itself (0 / 1 / NaN), the reference's (lat, lon, time) array.
#include "wagg_common.h"

namespace wagg {

constexpr int SR_NONE = 0, SR_POLY = 1, SR_EDD = 2;
constexpr int SR_MAX_PLANES = 4;
constexpr int SR_UNROLL = 4;                // (= PR_UNROLL of wagg_period.hip)
constexpr int SR_BLOCK = 256;
constexpr int SR_TARGET_BLOCKS = 1024;      // 256 CUs x 4: below this a period's rows are split
constexpr int SR_MAX_SPLIT = 64;
constexpr int SR_MIN_ROWS_PER_PART = 8;
constexpr int32_t SR_WIN_NULL = 1 << 21, SR_WIN_INVERT = 1 << 20;

template <typename T> struct SeasonXf {
    T off;
    int pow_first, planes;
    T thr[SR_MAX_PLANES];
};

struct SeasonShape {
    int64_t T, n, ldx, n_rows;
    int32_t P, n_colblk, split, reserved0;
};

// is day-of-year d inside the packed window w?  (a null window and a day outside 0..1023 are in no season)
__device__ __forceinline__ bool in_season(int32_t d, int32_t w) {
    const int32_t a = w & 1023, b = (w >> 10) & 1023;
    const bool inside = d >= a && d <= b;
    return (w & SR_WIN_NULL) == 0 && (uint32_t)d <= 1023u && inside != ((w & SR_WIN_INVERT) != 0);
}

// the cells [col, col + VEC) of one row; a piece that would reach past n is read cell by cell (cells past n read 0)
template <typename T, int VEC>
__device__ __forceinline__ void season_load_piece(const T *__restrict__ row, int64_t col, int64_t n, T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = row[col];
    } else {
        typedef T vec_t __attribute__((ext_vector_type(VEC)));
        if (col + VEC <= n) {
            const vec_t x = *reinterpret_cast<const vec_t *>(row + col);
#pragma unroll
            for (int c = 0; c < VEC; ++c) v[c] = x[c];
        } else {
#pragma unroll
            for (int c = 0; c < VEC; ++c) v[c] = col + c < n ? row[col + c] : T(0);
        }
    }
}

// VEC = 4 / 2 (16-byte pieces; needs 16-byte aligned rows) or 1 (any alignment).  Grid: n_colblk x P x split blocks, flat.
// DST = T: the finished sums go to `out`; DST = double: partial sums of part `s` go to `out` = the workspace
// [s][plane][p][j] (ldo = n, pstride = P * n), finished by season_finish_kernel.
template <typename T, int VEC, int MODE, typename DST>
__global__ void __launch_bounds__(SR_BLOCK)
season_reduce_kernel(const T *__restrict__ X, const T *__restrict__ X2, SeasonShape sh, const int32_t *__restrict__ row_begin,
                     const int32_t *__restrict__ rows, const int32_t *__restrict__ doy, const int32_t *__restrict__ win,
                     SeasonXf<T> xf, DST *__restrict__ out, int64_t ldo, int64_t pstride, int32_t *__restrict__ status) {
    constexpr int NPL = MODE == SR_NONE ? 1 : SR_MAX_PLANES;
    const int64_t blk = blockIdx.x;
    const int32_t cb = (int32_t)(blk % sh.n_colblk);
    const int64_t ps = blk / sh.n_colblk;
    const int32_t p = (int32_t)(ps % sh.P), s = (int32_t)(ps / sh.P);
    const int64_t col = ((int64_t)cb * SR_BLOCK + threadIdx.x) * VEC;
    // rows [b, e) of this block: part s of period p's list (a malformed row_begin is confined to the list's extent)
    int64_t b = row_begin[p], e = row_begin[p + 1];
    b = b < 0 ? 0 : (b > sh.n_rows ? sh.n_rows : b);
    e = e < b ? b : (e > sh.n_rows ? sh.n_rows : e);
    if (sh.split > 1) {
        const int64_t part = (e - b + sh.split - 1) / sh.split;
        b = b + part * s < e ? b + part * s : e;
        e = b + part < e ? b + part : e;
    }
    double acc[NPL][VEC];
#pragma unroll
    for (int k = 0; k < NPL; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc[k][c] = 0.0;
    bool saw_inf = false;
    if (col < sh.n) {
        int32_t w[VEC];                                          // the lane's windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) w[c] = col + c < sh.n ? win[col + c] : SR_WIN_NULL;
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
                    season_load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x[u]);
                    if constexpr (MODE == SR_EDD) season_load_piece<T, VEC>(X2 + t * sh.ldx, col, sh.n, x2[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < SR_UNROLL; ++u) {
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    T f[NPL];
                    if constexpr (MODE == SR_NONE) {
                        f[0] = x[u][c];
                    } else if constexpr (MODE == SR_POLY) {
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

// out[k][p][j] = (T) sum_s work[s][k][p][j], s ascending
template <typename T>
__global__ void season_finish_kernel(const double *__restrict__ work, int split, int planes, int64_t P, int64_t n, T *__restrict__ out,
                                     int64_t ldo, int64_t pstride) {
    const int64_t per = P * n, total = (int64_t)planes * per;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        double a = work[i];
        for (int s = 1; s < split; ++s) a += work[(int64_t)s * total + i];
        const int64_t k = i / per, r = i % per;
        out[k * pstride + (r / n) * ldo + r % n] = (T)a;
    }
}

// flag |= 1 unless row_begin ascends from >= 0 to <= n_rows and every listed row lies in [0, T)
__global__ void season_check_kernel(const int32_t *__restrict__ row_begin, int64_t P, const int32_t *__restrict__ rows, int64_t n_rows,
                                    int64_t T, int *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += stride)
        bad |= row_begin[i] < 0 || row_begin[i] > row_begin[i + 1] || row_begin[i + 1] > n_rows;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += stride)
        bad |= rows[i] < 0 || rows[i] >= T;
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// out[j][t] = NaN for a null window, else 1 / 0 as cell j is in season on day doy[t]
__global__ void season_mask_kernel(const int32_t *__restrict__ doy, int64_t T, const int32_t *__restrict__ win, int64_t n,
                                   double *__restrict__ out) {
    const int64_t total = n * T, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int32_t w = win[i / T], d = doy[i % T];
        out[i] = (w & SR_WIN_NULL) ? __builtin_nan("") : (in_season(d, w) ? 1.0 : 0.0);
    }
}

// how many consecutive parts a period's row list is cut into so that the grid fills the device (period_split's rule)
static int season_split(int64_t n, int64_t P, int64_t n_rows, int vec) {
    const int64_t n_colblk = (n + (int64_t)SR_BLOCK * vec - 1) / ((int64_t)SR_BLOCK * vec);
    const int64_t blocks = n_colblk * P;
    if (blocks <= 0 || blocks >= SR_TARGET_BLOCKS) return 1;
    int64_t want = (SR_TARGET_BLOCKS + blocks - 1) / blocks;
    const int64_t by_rows = n_rows / P / SR_MIN_ROWS_PER_PART;       // (mean list length: parts of a few rows are not worth a launch)
    if (want > by_rows) want = by_rows;
    if (want > SR_MAX_SPLIT) want = SR_MAX_SPLIT;
    return want < 2 ? 1 : (int)want;
}

template <typename T, int VEC, int MODE>
static void launch_season(const T *X, const T *X2, const SeasonShape &sh, const int32_t *row_begin, const int32_t *rows,
                          const int32_t *doy, const int32_t *win, const SeasonXf<T> &xf, T *out, int64_t ldo, int64_t pstride,
                          double *work, int32_t *status, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)sh.n_colblk * sh.P * sh.split)), block(SR_BLOCK);
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
    WAGG_REQUIRE(Ttot >= 0 && n >= 0 && P >= 0 && n_rows >= 0, "negative size (T=%lld, n=%lld, P=%d, n_rows=%lld)", (long long)Ttot,
                 (long long)n, (int)P, (long long)n_rows);
    WAGG_REQUIRE(Ttot <= 0x7fffffff && n_rows <= 0x7fffffff, "row indices are int32: T and n_rows must stay below 2^31");
    WAGG_REQUIRE(transform == WAGG_XF_NONE || transform == WAGG_XF_POLY || transform == WAGG_XF_EDD, "unknown transform %d", transform);
    WAGG_REQUIRE((flags & ~WAGG_PERIOD_ROWS_CHECKED) == 0, "unknown flags 0x%x (a season total has no keep-NaN form)", flags);
    int planes = 1;
    if (transform == WAGG_XF_POLY) {
        WAGG_REQUIRE(n_pow >= 1 && n_pow <= SR_MAX_PLANES && pow_first >= 1 && pow_first + n_pow - 1 <= 16,
                     "n_pow must be 1..%d and the powers 1..16 (pow_first=%d, n_pow=%d)", SR_MAX_PLANES, pow_first, n_pow);
        planes = n_pow;
    } else if (transform == WAGG_XF_EDD) {
        WAGG_REQUIRE(n_thr >= 1 && n_thr <= SR_MAX_PLANES, "n_thr must be 1..%d, got %d", SR_MAX_PLANES, n_thr);
        WAGG_REQUIRE(thresholds != nullptr, "thresholds is NULL");
        planes = n_thr;
    }
    WAGG_REQUIRE(ldx >= n && ldo >= n, "ldx / ldo smaller than n (ldx=%lld, ldo=%lld, n=%lld)", (long long)ldx, (long long)ldo, (long long)n);
    WAGG_REQUIRE(planes == 1 || pstride >= (int64_t)P * ldo, "out_pstride smaller than P * ldo");
    WAGG_REQUIRE(work_bytes >= 0 && (reinterpret_cast<uintptr_t>(work) & 7) == 0, "work_dev must be 8-byte aligned, work_bytes >= 0");
    WAGG_REQUIRE(status != nullptr && row_begin != nullptr, "NULL pointer (status_dev / row_begin)");
    WAGG_REQUIRE(n_rows == 0 || rows != nullptr, "NULL pointer (rows)");
    WAGG_REQUIRE(Ttot == 0 || doy != nullptr, "NULL pointer (doy_dev)");
    WAGG_REQUIRE(n == 0 || win != nullptr, "NULL pointer (win_dev)");
    if (P == 0 || n == 0) return WAGG_OK;
    WAGG_REQUIRE(out != nullptr, "NULL pointer (out_dev)");
    WAGG_REQUIRE(n_rows == 0 || Ttot == 0 || (X != nullptr && (transform != WAGG_XF_EDD || X2 != nullptr)), "NULL pointer (X_dev / X2_dev)");
    hipStream_t st = (hipStream_t)stream;
    if (!(flags & WAGG_PERIOD_ROWS_CHECKED)) {                   // one blocking look at the lists, as wagg_period_reduce_* takes it
        DevBuf<int> flag;
        int bad = 0;
        WAGG_HIP(flag.alloc(1));
        WAGG_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(season_check_kernel, dim3(256), dim3(256), 0, st, row_begin, (int64_t)P, rows, n_rows, Ttot, flag.p);
        WAGG_HIP(hipGetLastError());
        WAGG_HIP(staged_d2h(&bad, flag.p, sizeof(int), st));
        WAGG_REQUIRE(bad == 0, "row lists: row_begin must ascend within [0, n_rows] and every row index lie in [0, T)");
    }
    constexpr int V = 16 / (int)sizeof(T);
    const bool wide = ldx % V == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 &&
                      (transform != WAGG_XF_EDD || (reinterpret_cast<uintptr_t>(X2) & 15) == 0);
    const int vec = wide ? V : 1;
    SeasonShape sh;
    sh.T = Ttot; sh.n = n; sh.ldx = ldx; sh.n_rows = n_rows; sh.P = P; sh.reserved0 = 0;
    sh.n_colblk = (int32_t)((n + (int64_t)SR_BLOCK * vec - 1) / ((int64_t)SR_BLOCK * vec));
    int split = season_split(n, P, n_rows, vec);
    const int64_t per_part = 8 * (int64_t)planes * P * n;
    if (split > 1 && (work == nullptr || work_bytes / per_part < 2)) split = 1;
    if (split > 1 && work_bytes / per_part < split) split = (int)(work_bytes / per_part);
    sh.split = split;
    WAGG_REQUIRE((int64_t)sh.n_colblk * P * split < (int64_t)0x7fffffff, "too many pieces x periods for one launch");
    SeasonXf<T> xf;
    xf.off = (T)offset; xf.pow_first = pow_first; xf.planes = planes;
    for (int k = 0; k < SR_MAX_PLANES; ++k) xf.thr[k] = (T)(transform == WAGG_XF_EDD && k < n_thr ? thresholds[k] : 0.0);
    double *w = static_cast<double *>(work);
#define WAGG_SR_LAUNCH(VEC, MODE) launch_season<T, VEC, MODE>(X, X2, sh, row_begin, rows, doy, win, xf, out, ldo, pstride, w, status, st)
    if (wide) {
        if (transform == WAGG_XF_NONE) WAGG_SR_LAUNCH(V, SR_NONE);
        else if (transform == WAGG_XF_POLY) WAGG_SR_LAUNCH(V, SR_POLY);
        else WAGG_SR_LAUNCH(V, SR_EDD);
    } else {
        if (transform == WAGG_XF_NONE) WAGG_SR_LAUNCH(1, SR_NONE);
        else if (transform == WAGG_XF_POLY) WAGG_SR_LAUNCH(1, SR_POLY);
        else WAGG_SR_LAUNCH(1, SR_EDD);
    }
#undef WAGG_SR_LAUNCH
    WAGG_HIP(hipGetLastError());
    if (split > 1) {
        const int64_t total = (int64_t)planes * P * n;
        const int64_t nb = (total + 255) / 256;
        hipLaunchKernelGGL((season_finish_kernel<T>), dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, st, w, split, planes, (int64_t)P, n,
                           out, ldo, pstride);
        WAGG_HIP(hipGetLastError());
    }
    return WAGG_OK;
}

}  // namespace wagg

extern "C" int64_t wagg_season_reduce_work_bytes(int64_t n, int32_t P, int64_t n_rows, int planes) {
    if (n <= 0 || P <= 0 || n_rows <= 0 || planes <= 0) return 0;
    int s = wagg::season_split(n, P, n_rows, 1);                 // (the scalar path has more column blocks: never below the wide one)
    const int s4 = wagg::season_split(n, P, n_rows, 4);
    if (s4 > s) s = s4;
    return s > 1 ? 8 * (int64_t)s * planes * P * n : 0;
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
