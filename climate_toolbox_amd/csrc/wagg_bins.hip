// Temperature-bin day counts (wagg_bin_days_reduce_*): out[k][p][j] = the number of rows t of period p's list on which cell j is
// in season and edges[k] <= X[t, j] + offset < edges[k + 1], for up to WAGG_BIN_EDGES_MAX - 1 = 64 bins in ONE launch -- the
// third temperature statistic of climate-impact regressions beside the polynomials and the degree days.  Binning the grid on
// the host, or one 0/1 field per bin in front of an apply, is one pass over the field per bin.
//
// THE COMPARISON RULE.  Nothing is shifted in the element type.  The host forms c_k = edges[k] - offset in fp64 and hands the
// kernel ceilT(c_k), the smallest value of the element type that is not below c_k (fp32: (float)c, one nextafterf upward if
// that came out below c; infinities pass through; fp64: c itself).  The kernel compares the RAW X[t, j] against these: for
// every representable x, x >= ceilT(c) holds exactly when (double)x >= c, so an fp32 Kelvin field is binned as its exact values
// would be in fp64 and no value near an edge can flip.  Two edges between which no value of the type lies get one threshold: the
// bin between them is empty here as it is in fp64.
//
// The shape is the row-list family's (wagg_rowlist.h) and the season handling is edd_ladder_kernel's: a value out of season is
// selected away (it reaches neither a count nor the status word), a piece none of whose cells is in season is not read, an
// in-season +-inf sets bit 0 of the status word; with doy_dev = win_dev = NULL every listed row counts.  A lane counts, per edge
// of its group, the rows with x >= threshold in a 32-bit integer (the thresholds are wave-uniform: scalar registers) and
// differences adjacent counts at the end: bin k = count(x >= c_k) - count(x >= c_k+1), exact because the thresholds ascend.
// NaN compares false everywhere: it is in no bin (S6: it counts 0).  -inf passes a -inf first threshold only: an open-bottom
// first bin.  +inf passes every threshold, a +inf last one too: the differences are 0, it is in no bin.  A split list writes
// its differences as fp64 to the workspace and rowlist_finish adds the parts: integers far below 2^53, so every split gives
// the same bits, and the result is the count itself in the element type (exact in fp32 up to 2^24 days).  No atomics on a
// count, no LDS.
//
// The bins are cut into groups of BD_G = WAGG_BIN_GROUP = 8 (nine thresholds), the group being one more grid dimension beside
// column block x period x part, as EL_G is for the ladders; every group reads the field again.  BD_UNROLL = 2 rows in flight.
// hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage (VGPRs / scratch bytes / waves per SIMD; the season
// kernels, the no-season ones take 1-13 registers fewer; DST does not matter):
//   fp32 VEC = 4   74 / 0 / 6        fp32 VEC = 1   32 / 0 / 8        fp64 VEC = 2   56 / 0 / 8        fp64 VEC = 1   34 / 0 / 8
// No AGPRs, no LDS, no SGPR spilled either.  Groups of 16 bins would halve the passes over the field, but the 17 thresholds
// beside the in-season masks of the rows in flight no longer fit the scalar file: at 4 rows in flight fp32 VEC = 4 took 136
// registers = 3 waves with 27 SGPRs spilled to vector lanes, at 2 rows 101 registers = 4 waves with 14 spilled; 8 bins at 4
// rows still spilled 11 (89 registers, 5 waves).  A compare and an add per cell and edge: from a few bins on the kernel is
// bound by its passes over the field, not by arithmetic -- reasoning, not measurement.
#include "wagg_rowlist.h"

#include <cmath>

namespace wagg {

constexpr int BD_G = WAGG_BIN_GROUP;
constexpr int BD_UNROLL = 2;

template <typename T> struct BinThresholds {
    int n_edges;
    T c[WAGG_BIN_EDGES_MAX];
};

// SEASON = false: doy / win are not read, every valid listed row counts.  DST = T: the finished counts go to `out`; DST = double:
// the counts of part `s` go to `out` = the workspace (ldo = n, pstride = P * n), finished by rowlist_finish.
template <typename T, int VEC, bool SEASON, typename DST>
__global__ void __launch_bounds__(RL_BLOCK)
bin_days_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
                const int32_t *__restrict__ doy, const int32_t *__restrict__ win, BinThresholds<T> xf, DST *__restrict__ out, int64_t ldo,
                int64_t pstride, int32_t *__restrict__ status) {
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = (int32_t)(sg % sh.split), k0 = (int32_t)(sg / sh.split) * BD_G;
    const int n_bins = xf.n_edges - 1;
    const int kg = n_bins - k0 < BD_G ? n_bins - k0 : BD_G;          // bins of this group (>= 1 by the grid's extent)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    T thr[BD_G + 1];                                                 // (wave-uniform: scalar registers)
#pragma unroll
    for (int k = 0; k <= BD_G; ++k) thr[k] = xf.c[k0 + k <= n_bins ? k0 + k : n_bins];      // (a ragged group repeats the last edge)
    int32_t cnt[BD_G + 1][VEC];                                      // rows with x >= thr[k]
#pragma unroll
    for (int k = 0; k <= BD_G; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) cnt[k][c] = 0;
    bool saw_inf = false;
    if (col < sh.n) {
        int32_t w[VEC];                                              // the lane's windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (SEASON) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
            else w[c] = 0;
        }
        for (int64_t i = b; i < e; i += BD_UNROLL) {
            T x[BD_UNROLL][VEC];
            bool in[BD_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < BD_UNROLL; ++u) {
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
                    x[u][c] = T(0);
                }
                if (any) load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x[u]);      // no cell of this piece in season: no load
            }
#pragma unroll
            for (int u = 0; u < BD_UNROLL; ++u)
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    saw_inf |= in[u][c] && __builtin_isinf(x[u][c]);
                    const T v = in[u][c] ? x[u][c] : (T)__builtin_nan("");       // selected away: NaN passes no threshold
#pragma unroll
                    for (int k = 0; k <= BD_G; ++k) cnt[k][c] += v >= thr[k] ? 1 : 0;
                }
        }
#pragma unroll
        for (int k = 0; k < BD_G; ++k) {
            if (k >= kg) continue;
            DST *o = out + (int64_t)s * n_bins * pstride + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
#pragma unroll
            for (int c = 0; c < VEC; ++c)
                if (col + c < sh.n) o[c] = (DST)(cnt[k][c] - cnt[k + 1][c]);
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

template <typename T>
static int bin_days_reduce(const GroupedArgs<T> &a, double offset, const double *edges, int n_edges) {
    static const GroupedFamily fam = {"a bin count", "X_dev", 1, BD_G};
    return grouped_reduce<T>(
        fam, a, (int)((int64_t)n_edges - 1),                         // (the bins; not looked at unless n_edges passes the check)
        [&]() -> int {
            WAGG_REQUIRE(n_edges >= 2 && n_edges <= WAGG_BIN_EDGES_MAX, "n_edges must be 2..%d, got %d", WAGG_BIN_EDGES_MAX, n_edges);
            WAGG_REQUIRE(edges != nullptr, "edges is NULL");
            WAGG_REQUIRE(std::isfinite(offset), "offset must be finite");
            for (int k = 0; k < n_edges; ++k) {
                WAGG_REQUIRE(edges[k] == edges[k], "edge %d is NaN", k);
                WAGG_REQUIRE(k == 0 || edges[k] > edges[k - 1], "edges must ascend strictly (edge %d does not exceed edge %d)", k, k - 1);
            }
            return WAGG_OK;
        },
        [&](const RowlistShape &sh, bool wide, hipStream_t st) {
            BinThresholds<T> xf;
            xf.n_edges = n_edges;
            for (int k = 0; k < WAGG_BIN_EDGES_MAX; ++k) xf.c[k] = ceil_to<T>(edges[k < n_edges ? k : n_edges - 1] - offset);
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3 grid, auto *out, int64_t ldo, int64_t pstride) {
                using DST = std::remove_pointer_t<decltype(out)>;
                hipLaunchKernelGGL((bin_days_kernel<T, decltype(vec)::value, decltype(season)::value, DST>), grid, dim3(RL_BLOCK), 0, st,
                                   a.X, sh, a.row_begin, a.rows, a.doy, a.win, xf, out, ldo, pstride, a.status);
            });
        });
}

}  // namespace wagg

extern "C" int64_t wagg_bin_days_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_edges) {
    return wagg::rowlist_work_bytes(n, P, n_rows, n_edges - 1);
}

extern "C" int wagg_bin_days_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                        const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                        double offset, const double *edges, int n_edges, int flags, float *out_dev, int64_t ldo,
                                        int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::bin_days_reduce<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev,
                                         ldo, out_pstride, status_dev, work_dev, work_bytes, stream}, offset, edges, n_edges);
}
extern "C" int wagg_bin_days_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                        const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                        double offset, const double *edges, int n_edges, int flags, double *out_dev, int64_t ldo,
                                        int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::bin_days_reduce<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev,
                                          ldo, out_pstride, status_dev, work_dev, work_bytes, stream}, offset, edges, n_edges);
}
