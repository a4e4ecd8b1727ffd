// Period totals (wagg_period_reduce_*): out[k][p][j] = sum over the rows t of period p, in list order, of f_k(X[t, j]).
// The sum over time is linear, so it can run in FRONT of the aggregation (on the field: the contraction then sees P rows
// instead of T) or BEHIND it (on the (T x R) result, so that (P x R) leaves the device): climate_toolbox_amd/periods.py.
//
// The base of the row-list family (wagg_rowlist.h has the shape): bound by the one read of X, PR_UNROLL loads in flight;
// period and row bookkeeping is the same in every lane of a block, so it stays in scalar registers.  fp32 and fp64 data both
// accumulate in fp64, rounded once at the end.  Particular to this kernel: keep_nan, and an invalid row skipped by branch.
// The family's host pieces -- split rule, list check, finish, geometry, the shared argument checks -- are defined here.
#include "wagg_rowlist.h"

namespace wagg {

constexpr int PR_UNROLL = 4;

// DST = T: the finished sums go to `out`; DST = double: partial sums of part `s` go to `out` = the workspace (ldo = n,
// pstride = P * n), finished by rowlist_finish.
template <typename T, int VEC, int MODE, typename DST>
__global__ void __launch_bounds__(RL_BLOCK)
period_reduce_kernel(const T *__restrict__ X, const T *__restrict__ X2, RowlistShape sh, const int32_t *__restrict__ row_begin,
                     const int32_t *__restrict__ rows, RowlistXf<T> xf, DST *__restrict__ out, int64_t ldo, int64_t pstride,
                     int32_t *__restrict__ status) {
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
        for (int64_t i = b; i < e; i += PR_UNROLL) {
            T x[PR_UNROLL][VEC], x2[PR_UNROLL][VEC];
            bool ok[PR_UNROLL];
#pragma unroll
            for (int u = 0; u < PR_UNROLL; ++u) {
                const int64_t t = i + u < e ? (int64_t)rows[i + u] : -1;
                ok[u] = t >= 0 && t < sh.T;                    // (wave-uniform; a row index outside the field is never read)
                if (ok[u]) {
                    load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x[u]);
                    if constexpr (MODE == RL_EDD) load_piece<T, VEC>(X2 + t * sh.ldx, col, sh.n, x2[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < PR_UNROLL; ++u) {
                if (!ok[u]) continue;
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
                        T v = f[k];
                        saw_inf |= __builtin_isinf(v);
                        if (!sh.aux && v != v) v = T(0);         // S6: a NaN term counts 0 (aux = keep_nan)
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

template <typename T>
__global__ void rowlist_finish_kernel(const double *__restrict__ work, int split, int planes, int64_t P, int64_t n, T *__restrict__ out,
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

template <typename T>
int rowlist_finish(const double *work, int split, int planes, int64_t P, int64_t n, T *out, int64_t ldo, int64_t pstride, hipStream_t st) {
    if (split <= 1) return WAGG_OK;
    const int64_t nb = ((int64_t)planes * P * n + 255) / 256;
    hipLaunchKernelGGL((rowlist_finish_kernel<T>), dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, st, work, split, planes, P, n, out,
                       ldo, pstride);
    WAGG_HIP(hipGetLastError());
    return WAGG_OK;
}
template int rowlist_finish<float>(const double *, int, int, int64_t, int64_t, float *, int64_t, int64_t, hipStream_t);
template int rowlist_finish<double>(const double *, int, int, int64_t, int64_t, double *, int64_t, int64_t, hipStream_t);

// flag |= 1 unless row_begin ascends from >= 0 to <= n_rows and every listed row lies in [0, T)
__global__ void rowlist_check_kernel(const int32_t *__restrict__ row_begin, int64_t P, const int32_t *__restrict__ rows, int64_t n_rows,
                                     int64_t T, int *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += stride)
        bad |= row_begin[i] < 0 || row_begin[i] > row_begin[i + 1] || row_begin[i + 1] > n_rows;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += stride)
        bad |= rows[i] < 0 || rows[i] >= T;
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

int rowlist_check_rows(const int32_t *row_begin, int32_t P, const int32_t *rows, int64_t n_rows, int64_t T, int flags, hipStream_t st) {
    if (flags & WAGG_PERIOD_ROWS_CHECKED) return WAGG_OK;
    DevBuf<int> flag;                                            // (blocking; any_less does the same)
    int bad = 0;
    WAGG_HIP(flag.alloc(1));
    WAGG_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(rowlist_check_kernel, dim3(256), dim3(256), 0, st, row_begin, (int64_t)P, rows, n_rows, T, flag.p);
    WAGG_HIP(hipGetLastError());
    WAGG_HIP(staged_d2h(&bad, flag.p, sizeof(int), st));
    WAGG_REQUIRE(bad == 0, "row lists: row_begin must ascend within [0, n_rows] and every row index lie in [0, T)");
    return WAGG_OK;
}

int rowlist_require_sizes(int64_t T, int64_t n, int32_t P, int64_t n_rows) {
    WAGG_REQUIRE(T >= 0 && n >= 0 && P >= 0 && n_rows >= 0, "negative size (T=%lld, n=%lld, P=%d, n_rows=%lld)", (long long)T, (long long)n,
                 (int)P, (long long)n_rows);
    WAGG_REQUIRE(T <= 0x7fffffff && n_rows <= 0x7fffffff, "row indices are int32: T and n_rows must stay below 2^31");
    return WAGG_OK;
}

int rowlist_require_layout(int64_t n, int64_t ldx, int64_t ldo, int32_t P, int planes, int64_t pstride, const void *work,
                           int64_t work_bytes, const void *status, const void *row_begin, const void *rows, int64_t n_rows) {
    WAGG_REQUIRE(ldx >= n && ldo >= n, "ldx / ldo smaller than n (ldx=%lld, ldo=%lld, n=%lld)", (long long)ldx, (long long)ldo, (long long)n);
    WAGG_REQUIRE(planes == 1 || pstride >= (int64_t)P * ldo, "out_pstride smaller than P * ldo");
    WAGG_REQUIRE(work_bytes >= 0 && (reinterpret_cast<uintptr_t>(work) & 7) == 0, "work_dev must be 8-byte aligned, work_bytes >= 0");
    WAGG_REQUIRE(status != nullptr && row_begin != nullptr, "NULL pointer (status_dev / row_begin)");
    WAGG_REQUIRE(n_rows == 0 || rows != nullptr, "NULL pointer (rows)");
    return WAGG_OK;
}

static int64_t rowlist_colblk(int64_t n, int vec) { return (n + (int64_t)RL_BLOCK * vec - 1) / ((int64_t)RL_BLOCK * vec); }

int rowlist_split(int64_t n, int64_t P, int64_t n_rows, int vec) {
    const int64_t blocks = rowlist_colblk(n, vec) * P;
    if (blocks <= 0 || blocks >= RL_TARGET_BLOCKS) return 1;
    int64_t want = (RL_TARGET_BLOCKS + blocks - 1) / blocks;
    const int64_t by_rows = n_rows / P / RL_MIN_ROWS_PER_PART;       // (mean list length: parts of a few rows are not worth a launch)
    if (want > by_rows) want = by_rows;
    if (want > RL_MAX_SPLIT) want = RL_MAX_SPLIT;
    return want < 2 ? 1 : (int)want;
}

int64_t rowlist_work_bytes(int64_t n, int64_t P, int64_t n_rows, int planes) {
    if (n <= 0 || P <= 0 || n_rows <= 0 || planes <= 0) return 0;
    int s = rowlist_split(n, P, n_rows, 1);                      // (the scalar path has more column blocks: never below the wide one)
    const int s4 = rowlist_split(n, P, n_rows, 4);
    if (s4 > s) s = s4;
    return s > 1 ? 8 * (int64_t)s * planes * P * n : 0;
}

bool rowlist_geometry(RowlistShape &sh, bool &wide, int elem_bytes, const void *X, const void *X2, int planes, const void *work,
                      int64_t work_bytes, int n_grp) {
    const int V = 16 / elem_bytes;
    wide = sh.ldx % V == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(X2) & 15) == 0;
    const int vec = wide ? V : 1;
    sh.n_colblk = (int32_t)rowlist_colblk(sh.n, vec);
    int split = rowlist_split(sh.n, sh.P, sh.n_rows, vec);
    const int64_t per_part = 8 * (int64_t)planes * sh.P * sh.n;
    if (split > 1 && (work == nullptr || work_bytes / per_part < 2)) split = 1;
    if (split > 1 && work_bytes / per_part < split) split = (int)(work_bytes / per_part);
    sh.split = split;
    return (int64_t)sh.n_colblk * sh.P * split * n_grp < (int64_t)0x7fffffff;
}

template <typename T, int VEC, int MODE>
static void launch_reduce(const T *X, const T *X2, const RowlistShape &sh, const int32_t *row_begin, const int32_t *rows,
                          const RowlistXf<T> &xf, T *out, int64_t ldo, int64_t pstride, double *work, int32_t *status, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)sh.n_colblk * sh.P * sh.split)), block(RL_BLOCK);
    if (sh.split > 1)
        hipLaunchKernelGGL((period_reduce_kernel<T, VEC, MODE, double>), grid, block, 0, st, X, X2, sh, row_begin, rows, xf, work, sh.n,
                           (int64_t)sh.P * sh.n, status);
    else
        hipLaunchKernelGGL((period_reduce_kernel<T, VEC, MODE, T>), grid, block, 0, st, X, X2, sh, row_begin, rows, xf, out, ldo, pstride,
                           status);
}

template <typename T>
static int period_reduce(const T *X, const T *X2, int64_t Ttot, int64_t n, int64_t ldx, const int32_t *row_begin, const int32_t *rows,
                         int32_t P, int64_t n_rows, int transform, double offset, int pow_first, int n_pow, const double *thresholds,
                         int n_thr, int flags, T *out, int64_t ldo, int64_t pstride, int32_t *status, void *work, int64_t work_bytes,
                         void *stream) {
    clear_error();
    WAGG_TRY(rowlist_require_sizes(Ttot, n, P, n_rows));
    WAGG_REQUIRE(transform == WAGG_XF_NONE || transform == WAGG_XF_POLY || transform == WAGG_XF_EDD, "unknown transform %d", transform);
    WAGG_REQUIRE((flags & ~(WAGG_PERIOD_KEEP_NAN | WAGG_PERIOD_ROWS_CHECKED)) == 0, "unknown flags 0x%x", flags);
    RowlistXf<T> xf;
    WAGG_TRY(rowlist_xf<T>(transform, offset, pow_first, n_pow, thresholds, n_thr, xf));
    WAGG_TRY(rowlist_require_layout(n, ldx, ldo, P, xf.planes, pstride, work, work_bytes, status, row_begin, rows, n_rows));
    if (P == 0 || n == 0) return WAGG_OK;
    WAGG_REQUIRE(out != nullptr, "NULL pointer (out_dev)");
    WAGG_REQUIRE(n_rows == 0 || Ttot == 0 || (X != nullptr && (transform != WAGG_XF_EDD || X2 != nullptr)), "NULL pointer (X_dev / X2_dev)");
    hipStream_t st = (hipStream_t)stream;
    WAGG_TRY(rowlist_check_rows(row_begin, P, rows, n_rows, Ttot, flags, st));
    RowlistShape sh;
    sh.T = Ttot; sh.n = n; sh.ldx = ldx; sh.n_rows = n_rows; sh.P = P;
    sh.aux = (flags & WAGG_PERIOD_KEEP_NAN) ? 1 : 0;
    bool wide;
    WAGG_REQUIRE(rowlist_geometry(sh, wide, (int)sizeof(T), X, transform == WAGG_XF_EDD ? X2 : nullptr, xf.planes, work, work_bytes),
                 "too many pieces x periods for one launch");
    constexpr int V = 16 / (int)sizeof(T);
    double *w = static_cast<double *>(work);
#define WAGG_PR_LAUNCH(VEC, MODE) launch_reduce<T, VEC, MODE>(X, X2, sh, row_begin, rows, xf, out, ldo, pstride, w, status, st)
    if (wide) {
        if (transform == WAGG_XF_NONE) WAGG_PR_LAUNCH(V, RL_NONE);
        else if (transform == WAGG_XF_POLY) WAGG_PR_LAUNCH(V, RL_POLY);
        else WAGG_PR_LAUNCH(V, RL_EDD);
    } else {
        if (transform == WAGG_XF_NONE) WAGG_PR_LAUNCH(1, RL_NONE);
        else if (transform == WAGG_XF_POLY) WAGG_PR_LAUNCH(1, RL_POLY);
        else WAGG_PR_LAUNCH(1, RL_EDD);
    }
#undef WAGG_PR_LAUNCH
    WAGG_HIP(hipGetLastError());
    return rowlist_finish<T>(w, sh.split, xf.planes, P, n, out, ldo, pstride, st);
}

}  // namespace wagg

extern "C" int64_t wagg_period_reduce_work_bytes(int64_t n, int32_t P, int64_t n_rows, int planes) {
    return wagg::rowlist_work_bytes(n, P, n_rows, planes);
}

extern "C" int wagg_period_reduce_f32(const float *X_dev, const float *X2_dev, int64_t T, int64_t n, int64_t ldx,
                                      const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows, int transform,
                                      double offset, int pow_first, int n_pow, const double *thresholds, int n_thr, int flags,
                                      float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                                      int64_t work_bytes, void *stream) {
    return wagg::period_reduce<float>(X_dev, X2_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, transform, offset, pow_first, n_pow,
                                      thresholds, n_thr, flags, out_dev, ldo, out_pstride, status_dev, work_dev, work_bytes, stream);
}
extern "C" int wagg_period_reduce_f64(const double *X_dev, const double *X2_dev, int64_t T, int64_t n, int64_t ldx,
                                      const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows, int transform,
                                      double offset, int pow_first, int n_pow, const double *thresholds, int n_thr, int flags,
                                      double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                                      int64_t work_bytes, void *stream) {
    return wagg::period_reduce<double>(X_dev, X2_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, transform, offset, pow_first, n_pow,
                                       thresholds, n_thr, flags, out_dev, ldo, out_pstride, status_dev, work_dev, work_bytes, stream);
}
