// Hinge totals (wagg_hinge_reduce_*): out[j][p][i] = sum over the rows t of period p, in list order, on which cell i is in
// season, of h(X[t, i]; knots[j]) with h(x; k) = max(+-((x + off) - k), 0)^power, for up to WAGG_HINGE_MAX knots in ONE launch --
// the fourth temperature statistic of climate-impact regressions beside the polynomials, the Snyder degree days and the bins:
// power 1 on the daily mean is cooling (side above) / heating (side below) degree days, power 1 at several knots a linear
// spline, power 3 the terms of a restricted cubic spline.  One clamped grid per knot in front of an apply is one pass over the
// field per knot.
//
// THE ARITHMETIC.  d = (x + off) - k is formed in the element type in exactly these two operations (contraction is off in the
// whole kernel, as in snyder_edd1_outside), negated for side "below"; the term is d > 0 ? d^power : 0 with d^2 = d * d and
// d^3 = (d * d) * d, in the element type; it is added to an fp64 sum per lane and knot.  A NaN compares false: it gives 0 (S6).
// +inf on the counted side gives +inf, -inf there gives 0; an IN-SEASON +-inf of the field sets bit 0 of the status word
// whichever side is asked for (one atomicOr per wave).  A power that overflows the element type from a finite value leaves +inf
// in its plane and sets nothing.
//
// THE TAIL (TAIL = true; the restricted cubic spline).  Every group also sums the hinges at two tail knots kA, kB, and plane j
// leaves the kernel as (acc_j + ca[j] * acc_A) + cb[j] * acc_B, in fp64, per part, before the cast or the workspace store: the
// cancellation of the spline's three cubes beyond the last knot happens among fp64 sums, not among fp32 results.  The
// combination is linear, so rowlist_finish still just adds the parts.  TAIL = false instances carry none of it.
//
// The shape is the row-list family's (wagg_rowlist.h) and the season handling is bin_days_kernel's: a value out of season is
// selected away (it reaches neither a sum nor the status word), a piece none of whose cells is in season is not read; with
// doy_dev = win_dev = NULL every listed row counts.  The knots are cut into groups of HG_G = WAGG_HINGE_GROUP = 8, the group
// being one more grid dimension beside column block x period x part, as EL_G is for the ladders; every group reads the field
// again.  The knots of a group, the power and the side are wave-uniform.  No LDS, no atomics on a sum.  A plane's sum depends
// on its own knot, the list and the split alone: a plane of a many-knot call is bit for bit the plane of the call with that
// knot alone (each with the workspace its own wagg_hinge_work_bytes reports: the split rule does not look at the planes),
// and an all-year window for every cell gives the bits of the call without a season.
//
// HG_UNROLL = 2 rows in flight, the siblings' depth: the sums are the ladder's (8 x VEC fp64, 10 x VEC with the tail), and
// the ladder at 4 rows left the 128 registers that 4 waves per SIMD allow.
// hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage (VGPRs / scratch bytes / waves per SIMD; the season
// kernels, without the tail | with it; the no-season ones take 1-5 registers fewer; DST does not matter):
//   fp32 VEC = 4    91 / 0 / 5 | 114 / 0 / 4      fp32 VEC = 1   48 / 0 / 8 | 74 / 0 / 6
//   fp64 VEC = 2    59 / 0 / 7 |  73 / 0 / 6      fp64 VEC = 1   40 / 0 / 7 | 40 / 0 / 7
// The wide season kernels keep some scalars in vector lanes (SGPRs spilled: fp32 VEC = 4 13 | 23, fp64 VEC = 2 2 | 10; the
// no-season ones 0-4, every VEC = 1 instance 0): no scratch memory is involved.  Selecting the out-of-season values away ahead
// of the knot loop, so that no mask is held across it, compiled to the same registers and the same spills.
// No AGPRs, no LDS.  Two subtractions, a compare, a select, up to two multiplications, a conversion and an fp64 add per cell and
// knot: like the ladder, from a few knots on the kernel should be bound by arithmetic (the fp64 adds), not by its loads --
// reasoning, not measurement.
#include "wagg_rowlist.h"

#include <cmath>

namespace wagg {

constexpr int HG_G = WAGG_HINGE_GROUP;
constexpr int HG_UNROLL = 2;

template <typename T> struct HingeXf {
    T off;
    int n_knots, power, below;
    T k[WAGG_HINGE_MAX];
    T tail[2];                                  // TAIL kernels only, like ca / cb
    double ca[WAGG_HINGE_MAX], cb[WAGG_HINGE_MAX];
};

// max(+-d, 0)^power for d = xo - k, xo = x + off; NaN gives 0
template <typename T> __device__ __forceinline__ T hinge_term(T xo, T k, int power, bool below) {
#pragma clang fp contract(off)
    T d = xo - k;
    d = below ? -d : d;
    const T d2 = d * d;
    const T t = power == 1 ? d : (power == 2 ? d2 : d2 * d);
    return d > T(0) ? t : T(0);
}

// SEASON = false: doy / win are not read, every valid listed row counts.  DST = T: the finished sums go to `out`; DST = double:
// the sums of part `s` go to `out` = the workspace (ldo = n, pstride = P * n), finished by rowlist_finish.
template <typename T, int VEC, bool SEASON, bool TAIL, typename DST>
__global__ void __launch_bounds__(RL_BLOCK)
hinge_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
             const int32_t *__restrict__ doy, const int32_t *__restrict__ win, HingeXf<T> xf, DST *__restrict__ out, int64_t ldo,
             int64_t pstride, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = (int32_t)(sg % sh.split), k0 = (int32_t)(sg / sh.split) * HG_G;
    const int kg = xf.n_knots - k0 < HG_G ? xf.n_knots - k0 : HG_G;  // knots of this group (>= 1 by the grid's extent)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    constexpr int NK = TAIL ? HG_G + 2 : HG_G;                       // the group's knots, then kA and kB
    T knot[NK];                                                      // (wave-uniform: scalar registers)
#pragma unroll
    for (int k = 0; k < HG_G; ++k) knot[k] = k < kg ? xf.k[k0 + k] : T(0);
    if constexpr (TAIL) {
        knot[HG_G] = xf.tail[0];
        knot[HG_G + 1] = xf.tail[1];
    }
    const int power = xf.power;
    const bool below = xf.below != 0;
    double acc[NK][VEC];
#pragma unroll
    for (int k = 0; k < NK; ++k)
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
        for (int64_t i = b; i < e; i += HG_UNROLL) {
            T x[HG_UNROLL][VEC];
            bool in[HG_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < HG_UNROLL; ++u) {
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
            for (int u = 0; u < HG_UNROLL; ++u)
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    saw_inf |= in[u][c] && __builtin_isinf(x[u][c]);
                    const T v = in[u][c] ? x[u][c] : (T)__builtin_nan("");       // selected away: a NaN hinge is 0
                    const T xo = v + xf.off;
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        if (k < HG_G && k >= kg) continue;
                        acc[k][c] += (double)hinge_term<T>(xo, knot[k], power, below);
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < HG_G; ++k) {
            if (k >= kg) continue;
            DST *o = out + (int64_t)s * xf.n_knots * pstride + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
            double ca = 0.0, cb2 = 0.0;
            if constexpr (TAIL) {
                ca = xf.ca[k0 + k];
                cb2 = xf.cb[k0 + k];
            }
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                double r = acc[k][c];
                if constexpr (TAIL) r = (r + ca * acc[HG_G][c]) + cb2 * acc[HG_G + 1][c];
                if (col + c < sh.n) o[c] = (DST)r;
            }
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

template <typename T>
static int hinge_reduce(const GroupedArgs<T> &a, double offset, const double *knots, int n_knots, int power, int side,
                        const double *tail_knots, const double *tail_a, const double *tail_b) {
    static const GroupedFamily fam = {"a hinge total", "X_dev", 1, HG_G};
    const bool tail = tail_knots != nullptr;
    return grouped_reduce<T>(
        fam, a, n_knots,
        [&]() -> int {
            WAGG_REQUIRE(n_knots >= 1 && n_knots <= WAGG_HINGE_MAX, "n_knots must be 1..%d, got %d", WAGG_HINGE_MAX, n_knots);
            WAGG_REQUIRE(knots != nullptr, "knots is NULL");
            WAGG_REQUIRE(power >= 1 && power <= 3, "power must be 1..3, got %d", power);
            WAGG_REQUIRE(side == WAGG_HINGE_ABOVE || side == WAGG_HINGE_BELOW, "side must be WAGG_HINGE_ABOVE or WAGG_HINGE_BELOW, got %d",
                         side);
            WAGG_REQUIRE(std::isfinite(offset), "offset must be finite");
            for (int k = 0; k < n_knots; ++k) WAGG_REQUIRE(std::isfinite(knots[k]), "knot %d is not finite", k);
            WAGG_REQUIRE(tail == (tail_a != nullptr) && tail == (tail_b != nullptr),
                         "tail_knots, tail_a and tail_b go together: all given, or all NULL (no tail)");
            if (tail) {
                WAGG_REQUIRE(std::isfinite(tail_knots[0]) && std::isfinite(tail_knots[1]), "a tail knot is not finite");
                for (int k = 0; k < n_knots; ++k)
                    WAGG_REQUIRE(std::isfinite(tail_a[k]) && std::isfinite(tail_b[k]), "tail coefficient %d is not finite", k);
            }
            return WAGG_OK;
        },
        [&](const RowlistShape &sh, bool wide, hipStream_t st) {
            HingeXf<T> xf;
            xf.off = (T)offset; xf.n_knots = n_knots; xf.power = power; xf.below = side == WAGG_HINGE_BELOW;
            for (int k = 0; k < WAGG_HINGE_MAX; ++k) {
                xf.k[k] = (T)(k < n_knots ? knots[k] : 0.0);
                xf.ca[k] = tail && k < n_knots ? tail_a[k] : 0.0;
                xf.cb[k] = tail && k < n_knots ? tail_b[k] : 0.0;
            }
            xf.tail[0] = (T)(tail ? tail_knots[0] : 0.0);
            xf.tail[1] = (T)(tail ? tail_knots[1] : 0.0);
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3 grid, auto *out, int64_t ldo, int64_t pstride) {
                constexpr int VEC = decltype(vec)::value;
                constexpr bool SEASON = decltype(season)::value;
                using DST = std::remove_pointer_t<decltype(out)>;
                auto *kernel = tail ? hinge_kernel<T, VEC, SEASON, true, DST> : hinge_kernel<T, VEC, SEASON, false, DST>;
                hipLaunchKernelGGL(kernel, grid, dim3(RL_BLOCK), 0, st, a.X, sh, a.row_begin, a.rows, a.doy, a.win, xf, out, ldo, pstride,
                                   a.status);
            });
        });
}

}  // namespace wagg

extern "C" int64_t wagg_hinge_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_knots) {
    return wagg::rowlist_work_bytes(n, P, n_rows, n_knots);
}

extern "C" int wagg_hinge_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                     const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                     double offset, const double *knots, int n_knots, int power, int side, const double *tail_knots,
                                     const double *tail_a, const double *tail_b, int flags, float *out_dev, int64_t ldo,
                                     int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::hinge_reduce<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                      out_pstride, status_dev, work_dev, work_bytes, stream},
                                     offset, knots, n_knots, power, side, tail_knots, tail_a, tail_b);
}
extern "C" int wagg_hinge_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                     const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                     double offset, const double *knots, int n_knots, int power, int side, const double *tail_knots,
                                     const double *tail_a, const double *tail_b, int flags, double *out_dev, int64_t ldo,
                                     int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream) {
    return wagg::hinge_reduce<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                       out_pstride, status_dev, work_dev, work_bytes, stream},
                                      offset, knots, n_knots, power, side, tail_knots, tail_a, tail_b);
}
