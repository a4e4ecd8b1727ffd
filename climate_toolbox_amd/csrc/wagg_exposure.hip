// Sinusoid exposure bins (wagg_exposure_reduce_*): out[k][p][j] = sum over the rows t of period p, in list order, on which cell j
// is in season, of A(lo, hi, edges[k]) - A(lo, hi, edges[k + 1]),  lo = X[t, j] + off, hi = X2[t, j] + off, for up to
// WAGG_EXPOSURE_EDGES_MAX - 1 = 64 bins in ONE launch -- the time the day's single-sine temperature curve (the one snyder_edd1
// integrates) spends in each bin, the Schlenker-Roberts exposure bins.  A(lo, hi, e) is the fraction of the day above e,
// A = -d EDD / de:
//   0                          if lo or hi is NaN      (the day is in no bin; checked first)
//   1                          if !(lo < e)            (snyder_edd1's own comparisons, in its order)
//   0                          if !(hi > e)
//   clamp(acos(z) / pi, 0, 1)  otherwise,  z = (e - M) / w clamped to [-1, 1],  M = (hi + lo) / 2,  w = (hi - lo) / 2
// The two outer cases are selected, so they are exactly 1 and 0; inverted data (lo > hi) is a step at lo by the comparisons.
//
// The shape is the row-list family's (wagg_rowlist.h) and the frame is edd_ladder_kernel's: season windows read once per lane,
// two rows in flight, a value out of season selected away (it reaches neither a sum nor the status word), a piece none of
// whose cells is in season not read, an in-season +-inf in either field sets bit 0 of the status word; with doy_dev = win_dev =
// NULL every listed row counts.  No LDS, no atomics except that atomicOr.
//
// THE SUMS.  A lane sums the PER-DAY DIFFERENCES A(e_k) - A(e_k+1), formed in the element type, in one fp64 sum per bin -- not
// one sum per edge differenced at the end as bin_days_kernel does with its counts: nine per-edge sums of a group of eight bins
// are 72 registers for fp32 VEC = 4, eight per-bin sums 64, the ladder's budget.  Both A lie in [0, 1], so the difference
// rounds by at most eps / 2 of itself, and where both are selected (0 or 1) it is exact: a day wholly inside one bin adds
// exactly 1 to it.  The bins are cut into groups of EX_G = WAGG_EXPOSURE_GROUP = 8, the group being one more grid dimension
// beside column block x period x part; a group evaluates its EX_G + 1 edges, one after the other, keeping only the A of the
// edge before; every group reads its tasmin / tasmax pieces again (L2 serves what HBM served once).
//
// BAND SKIPPING.  Per edge and row a wave takes the ladder's ballot -- has ANY lane e strictly inside the range of its
// in-season cells, least lo to greatest hi?  No cell with lo < e < hi escapes that.  If none has, no acos is evaluated and each
// lane takes A from !(lo < e) alone (exposure1_outside): the value the full function selects, bit for bit, so a column's bins
// do not depend on what its neighbours in the wave hold.  On a 0..40 C set of edges most edges lie outside a cell's diurnal
// range on a given day.
//
// fp32 ARCCOSINE.  Not libm acosf behind an IEEE division per value; as in snyder_edd1_finite, ONE
// v_rcp_f32 (of w, once per day and cell, shared by the edges), one v_sqrt_f32 and a short polynomial per edge: with
// t = 1 - |z|,  acos(1 - t) / pi = sqrt(t) Q(t)  on [0, 1] and A(-z) = 1 - A(z).  t is NOT formed as 1 - |(e - M) / w|, which
// cancels where the sinusoid only touches the edge (hi one ulp above e: A = 3e-4, lost entirely when z rounds to 1), but from
// the nearer extreme: t = min(hi - e, e - lo) / w -- the same number, both differences exact or nearly so -- and the nearer
// extreme says which half (hi - e <= e - lo: z >= 0, A = sqrt(t) Q(t); else 1 minus that).  Q: degree-6 minimax fit
// (tools/fit_acos_poly.py), |error in A| <= 6.1e-8 with the coefficients rounded to fp32; the whole fp32 formula differs from
// the fp64 libm evaluation of the same lo / hi / e by <= 1.5e-7 on random days and <= 4e-9 on days within 256 ulps of tangency
// (bound asked: 1e-6; tolerance of the fp32 path: 1e-4 of the counted days).  fp64 calls libm acos on the clamped z.
//
// EX_G = 8 bins a group, EX_UNROLL = 2 rows in flight.  hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage
// (VGPRs / scratch bytes / waves per SIMD / SGPRs spilled to vector lanes; DST does not matter; the fp64 instances with DST = T
// and DST = double are one kernel, so the 2 dtypes x {wide, 1} x {season, none} x {T, double} are twelve kernels):
//                    fp32 VEC = 4        fp32 VEC = 1        fp64 VEC = 2        fp64 VEC = 1
//   season           123 / 0 / 4 / 32    55 / 0 / 7 / 5      121 / 0 / 4 / 31    89 / 0 / 5 / 17
//   no season        119 / 0 / 4 / 18    54 / 0 / 7 / 0      118 / 0 / 4 / 21    89 / 0 / 5 / 13
// 0 scratch bytes in every instance.  The scalar file is what is short: nine edges, the in-season and the no-NaN masks of the
// cells of two rows, the row-list state; what does not fit lives in lanes of a vector register (v_writelane / v_readlane), not
// in memory.
// No AGPRs, no LDS.  In band an edge costs a cell ~16 vector instructions in fp32 (two subtractions, min, multiply, two clamps,
// sqrt, six fused multiply-adds, the half and the two selections) against 3 out of band, beside the fp64 add of the
// difference; from a handful of bins on the kernel is bound by that arithmetic in the bands and by its passes over the two
// fields outside them -- reasoning, not measurement.
#include "wagg_rowlist.h"

#include <cmath>

namespace wagg {

constexpr int EX_G = WAGG_EXPOSURE_GROUP;
constexpr int EX_UNROLL = 2;

template <typename T> struct ExposureXf {
    T off;
    int n_edges;
    T e[WAGG_EXPOSURE_EDGES_MAX];
};

// what exposure1<T> selects when NOT lo < e < hi, for a day that holds no NaN: 1 where tasmin is not below the edge, else 0
template <typename T> __device__ __forceinline__ T exposure1_outside(T lo, T e) { return !(lo < e) ? T(1) : T(0); }

// the fraction of the day above e, for a day that holds no NaN; rw = 1 / w, w = (hi - lo) / 2 (looked at only in the band,
// where w > 0)
template <typename T> __device__ __forceinline__ T exposure1(T lo, T hi, T rw, T e);
template <> __device__ __forceinline__ float exposure1<float>(float lo, float hi, float rw, float e) {
    const float dlo = e - lo, dhi = hi - e;
    // 1 - |z| from the nearer extreme (NaN or inf * 0 from +-inf data: the clamps return a number)
    const float t = __builtin_fminf(__builtin_fmaxf(__builtin_fminf(dlo, dhi) * rw, 0.0f), 1.0f);
    float q = 0.0007166327559389174f;
    q = __builtin_fmaf(q, t, -0.0007944452809169888f);
    q = __builtin_fmaf(q, t, 0.0017373113660141826f);
    q = __builtin_fmaf(q, t, 0.002172010950744152f);
    q = __builtin_fmaf(q, t, 0.008501029573380947f);
    q = __builtin_fmaf(q, t, 0.03750920295715332f);
    q = __builtin_fmaf(q, t, 0.4501582086086273f);
    const float s = __builtin_amdgcn_sqrtf(t) * q;                     // acos(|z|) / pi
    const float a = __builtin_fminf(__builtin_fmaxf(dhi <= dlo ? s : 1.0f - s, 0.0f), 1.0f);
    return !(lo < e) ? 1.0f : (!(hi > e) ? 0.0f : a);
}
template <> __device__ __forceinline__ double exposure1<double>(double lo, double hi, double rw, double e) {
    if (!(lo < e)) return 1.0;
    if (!(hi > e)) return 0.0;
    const double M = (hi + lo) / 2.0, w = (hi - lo) / 2.0;
    const double z = __builtin_fmin(__builtin_fmax((e - M) / w, -1.0), 1.0);
    return __builtin_fmin(__builtin_fmax(acos(z) / 3.14159265358979323846, 0.0), 1.0);
}

// SEASON = false: doy / win are not read, every valid listed row counts.  DST = T: the finished sums go to `out`; DST = double:
// partial sums of part `s` go to `out` = the workspace (ldo = n, pstride = P * n), finished by rowlist_finish.
template <typename T, int VEC, bool SEASON, typename DST>
__global__ void __launch_bounds__(RL_BLOCK)
exposure_kernel(const T *__restrict__ X, const T *__restrict__ X2, RowlistShape sh, const int32_t *__restrict__ row_begin,
                const int32_t *__restrict__ rows, const int32_t *__restrict__ doy, const int32_t *__restrict__ win, ExposureXf<T> xf,
                DST *__restrict__ out, int64_t ldo, int64_t pstride, int32_t *__restrict__ status) {
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = (int32_t)(sg % sh.split), k0 = (int32_t)(sg / sh.split) * EX_G;
    const int n_bins = xf.n_edges - 1;
    const int kg = n_bins - k0 < EX_G ? n_bins - k0 : EX_G;          // bins of this group (>= 1 by the grid's extent)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    T thr[EX_G + 1];                                                 // (wave-uniform: scalar registers)
#pragma unroll
    for (int k = 0; k <= EX_G; ++k) thr[k] = xf.e[k0 + k <= n_bins ? k0 + k : n_bins];      // (a ragged group repeats the last edge)
    double acc[EX_G][VEC];                                           // bin k0 + k
#pragma unroll
    for (int k = 0; k < EX_G; ++k)
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
        for (int64_t i = b; i < e; i += EX_UNROLL) {
            T x[EX_UNROLL][VEC], x2[EX_UNROLL][VEC];
            bool in[EX_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < EX_UNROLL; ++u) {
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
            for (int u = 0; u < EX_UNROLL; ++u) {
                T lo[VEC], hi[VEC], rw[VEC];
                bool cnt[VEC];                                       // in season and no NaN: the day is in some bin
                // the lane's in-season cells as one range [least lo, greatest hi], as in edd_ladder_kernel: NaN compares
                // false, it neither widens the range nor is it in any band
                T lane_lo = __builtin_huge_val(), lane_hi = -__builtin_huge_val();
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    lo[c] = x[u][c] + xf.off;
                    hi[c] = x2[u][c] + xf.off;
                    if (in[u][c] && lo[c] < lane_lo) lane_lo = lo[c];
                    if (in[u][c] && hi[c] > lane_hi) lane_hi = hi[c];
                    saw_inf |= in[u][c] && (__builtin_isinf(lo[c]) || __builtin_isinf(hi[c]));
                    cnt[c] = in[u][c] && lo[c] == lo[c] && hi[c] == hi[c];
                    if constexpr (sizeof(T) == 4) rw[c] = __builtin_amdgcn_rcpf(0.5f * (hi[c] - lo[c]));
                    else rw[c] = T(0);                               // (fp64 divides in the band itself)
                }
                T prev[VEC];
#pragma unroll
                for (int k = 0; k <= EX_G; ++k) {
                    if (k > kg) continue;
                    const bool band = lane_lo < thr[k] && lane_hi > thr[k];      // may an in-season cell's sinusoid cross thr[k]?
                    T f[VEC];
                    if (__ballot(band) != 0ull) {                    // (wave-uniform branch)
#pragma unroll
                        for (int c = 0; c < VEC; ++c) f[c] = exposure1<T>(lo[c], hi[c], rw[c], thr[k]);
                    } else {                                         // no lane of the wave needs the arccosine
#pragma unroll
                        for (int c = 0; c < VEC; ++c) f[c] = exposure1_outside<T>(lo[c], thr[k]);
                    }
#pragma unroll
                    for (int c = 0; c < VEC; ++c) {
                        f[c] = cnt[c] ? f[c] : T(0);                 // selected, not multiplied: nothing out of season gets further
                        if (k > 0) acc[k - 1][c] += (double)(prev[c] - f[c]);
                        prev[c] = f[c];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < EX_G; ++k) {
            if (k >= kg) continue;
            DST *o = out + (int64_t)s * n_bins * pstride + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
#pragma unroll
            for (int c = 0; c < VEC; ++c)
                if (col + c < sh.n) o[c] = (DST)acc[k][c];
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

template <typename T>
static int exposure_reduce(const GroupedArgs<T> &a, double offset, const double *edges, int n_edges) {
    static const GroupedFamily fam = {"an exposure total", "tasmin_dev / tasmax_dev", 2, EX_G};
    return grouped_reduce<T>(
        fam, a, (int)((int64_t)n_edges - 1),                         // (the bins; not looked at unless n_edges passes the check)
        [&]() -> int {
            WAGG_REQUIRE(n_edges >= 2 && n_edges <= WAGG_EXPOSURE_EDGES_MAX, "n_edges must be 2..%d, got %d", WAGG_EXPOSURE_EDGES_MAX,
                         n_edges);
            WAGG_REQUIRE(edges != nullptr, "edges is NULL");
            WAGG_REQUIRE(std::isfinite(offset), "offset must be finite");
            for (int k = 0; k < n_edges; ++k) {
                WAGG_REQUIRE(edges[k] == edges[k], "edge %d is NaN", k);
                WAGG_REQUIRE(k == 0 || edges[k] > edges[k - 1], "edges must ascend strictly (edge %d does not exceed edge %d)", k, k - 1);
            }
            return WAGG_OK;
        },
        [&](const RowlistShape &sh, bool wide, hipStream_t st) {
            ExposureXf<T> xf;
            xf.off = (T)offset; xf.n_edges = n_edges;
            for (int k = 0; k < WAGG_EXPOSURE_EDGES_MAX; ++k) xf.e[k] = (T)edges[k < n_edges ? k : n_edges - 1];
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3 grid, auto *out, int64_t ldo, int64_t pstride) {
                using DST = std::remove_pointer_t<decltype(out)>;
                hipLaunchKernelGGL((exposure_kernel<T, decltype(vec)::value, decltype(season)::value, DST>), grid, dim3(RL_BLOCK), 0, st,
                                   a.X, a.X2, sh, a.row_begin, a.rows, a.doy, a.win, xf, out, ldo, pstride, a.status);
            });
        });
}

}  // namespace wagg

extern "C" int64_t wagg_exposure_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_edges) {
    return wagg::rowlist_work_bytes(n, P, n_rows, n_edges - 1);
}

extern "C" int wagg_exposure_reduce_f32(const float *tasmin_dev, const float *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                                        const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                                        const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *edges, int n_edges,
                                        int flags, float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                                        int64_t work_bytes, void *stream) {
    return wagg::exposure_reduce<float>({tasmin_dev, tasmax_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags,
                                         out_dev, ldo, out_pstride, status_dev, work_dev, work_bytes, stream}, offset, edges, n_edges);
}
extern "C" int wagg_exposure_reduce_f64(const double *tasmin_dev, const double *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                                        const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                                        const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *edges, int n_edges,
                                        int flags, double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                                        int64_t work_bytes, void *stream) {
    return wagg::exposure_reduce<double>({tasmin_dev, tasmax_dev, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags,
                                          out_dev, ldo, out_pstride, status_dev, work_dev, work_bytes, stream}, offset, edges, n_edges);
}
