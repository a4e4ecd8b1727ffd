// Period quantiles (wagg_quantile_select_*): the order statistics of a cell's daily values per period and season -- the median,
// the 5th / 95th / 99th percentile, R95p thresholds -- for up to WAGG_QUANT_MAX = 16 quantiles in ONE launch.  The first row-list
// statistic that is neither a sum nor a running state in registers: a cell's whole period has to be held at once, so this is the
// first row-list family that uses LDS.  On the grid it is a torch.quantile along time per period, without the (T, G) temporary.
//
// THE DEFINITION (include/wagg.h has the same text; tests/quantile_ref.py is its NumPy twin).  Cell j, period p: entry i of
// rows[row_begin[p] : row_begin[p + 1]] is VALID when t = rows[i] lies in [0, T), cell j is in season on doy[t] (when a season is
// given) and X[t, j] is not NaN.  Order and gaps do not matter, a row listed twice counts twice, an in-season +-inf is valid (and
// sets status bit 0).  m = the number of valid entries, v[0] <= ... <= v[m - 1] their raw elements sorted (-0.0 ahead of +0.0:
// equal as numbers).  For q[k]:  h = (double)(m - 1) * q[k] (one fp64 product),  lo = (int)floor(h),  g = h - (double)lo, and
//   WAGG_QUANT_LINEAR  r = g == 0 ? (double)v[lo] : (double)v[lo] + ((double)v[lo + 1] - (double)v[lo]) * g     (no fma)
//   WAGG_QUANT_LOWER   r = v[lo]          WAGG_QUANT_HIGHER  r = v[g == 0 ? lo : lo + 1]
// out[k][p][j] = (T)(r + offset), rounded once; m == 0 gives NaN.
//
// WHAT WAS BUILT.  A block of 256 lanes owns one 128-byte tile of a row (CELLS = 32 fp32 / 16 fp64 cells) and one period; the grid
// is ceil(n / CELLS) x P, flat.  Two phases with one __syncthreads() between them.
//   Phase 1, load: lane = cell + CELLS * r; the 256 lanes take SLOTS = 256 / CELLS (8 / 16) entries of the list per pass, CELLS
// consecutive lanes one row's 128 bytes with plain 4- / 8-byte loads -- no 16-byte pieces, so neither the alignment of X nor ldx
// picks an instance: the instances are T x SEASON, four in all.  The row index and its doy are read per entry by the CELLS lanes
// that load it (one address each: a broadcast, but per 32- / 16-lane group, not per wave as in rolling_kernel -- a wave holds 2 / 4
// entries here); a lane whose cell is out of season, or past n, issues no load, so a tile none of whose cells is in season on a
// row does not read it.  Every element goes to LDS as an ORDER-PRESERVING UNSIGNED KEY, laid out [entry][cell] (128 bytes an
// entry):  key = u ^ (sign ? ~0 : sign bit)  on the element's bits u; an invalid entry stores the all-ones key, which is the image
// of a NaN pattern only, so no valid value has it and invalid entries sort behind every valid one.
//   Phase 2, select: lane = cell + CELLS * slot; slot s serves quantiles s, s + SLOTS, ...  (fp32: 8 slots, two quantiles a lane
// at most; fp64: 16 slots, one).  One sweep over the cell's column counts m (keys that are not all-ones).  v[lo] is found by
// MSB-first bisection on the key bits, ONE BIT A SWEEP: 32 / 64 sweeps, each counting the keys that agree with the prefix found
// so far and have a 0 at the bit.  v[lo + 1] needs no second bisection: one more sweep (only when g != 0 and the method reads it)
// gives c_le = #{key <= key_lo} and the least key above key_lo; v[lo + 1] is v[lo] when lo + 1 < c_le (a tie), else that least
// key.  Quantiles of one lane do not share sweeps and a sweep takes one bit, not two: the simplest form, nothing else was tried.
// LDS traffic: a sweep reads entry i's 128 bytes with one ds_read_b32 / ds_read_b64 per wave: the 32 (16) cells of a 32-lane group
// hit 32 distinct banks / 16 distinct 8-byte words, the other slots of the wave read the same words (a broadcast, no conflict);
// phase 1's stores are one ds_write_b32 / _b64 with consecutive lanes on consecutive words.  That this is conflict-free is read off
// the bank rule, not measured with a counter.
//
// CONFINEMENT.  Dynamic LDS is 128 * max_rows bytes (max_rows <= WAGG_QUANT_ROWS_MAX = 1024: 128 KiB of the CU's 160 KiB; the
// attribute is raised once per kernel through allow_dynamic_lds).  A block whose list -- after row_begin is confined to [0, n_rows]
// as in every row-list kernel -- is longer than max_rows writes NaN to its period's cells in every plane, sets status bit 1 and
// touches no LDS at all.  Without WAGG_PERIOD_ROWS_CHECKED the host's blocking look at the lists rejects such a call first.
// A list is never split (an order statistic does not add across parts): work / work_bytes are ignored, there is no *_work_bytes.
//
// hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage (measured on the compiler; VGPRs / SGPRs / scratch bytes /
// static LDS / waves per SIMD by registers):
//   fp32  no season  40 / 103 / 0 / 0 / 7      season  40 / 103 / 0 / 0 / 7
//   fp64  no season  43 / 100 / 0 / 0 / 8      season  41 / 100 / 0 / 0 / 8
// No AGPRs.  Occupancy is set by LDS, not registers: a 366-entry year is 46 848 bytes, three blocks (12 waves) a CU; at 1024
// entries a block has the CU to itself (4 waves).  REASONING, NOT MEASURED: that a 128-byte tile is the right width (a 256-byte
// tile would halve the blocks and double LDS per block: one block a CU for a year; nobody has timed either), and that one bit per
// sweep is fast enough (about (33 | 65) x entries LDS reads per lane and quantile; two bits a sweep would halve the reads for three
// counters a sweep).  MEASURED: the results against the NumPy restatement, exactly (tests/test_gpu_quantile.py), and the timings of
// tools/quantile_timing.py where profiles/quantile_timing.json exists.
#include "wagg_rowlist.h"

#include <cmath>

namespace wagg {

struct QuantXf {
    int n_q, method;
    int32_t max_rows;
    double offset;
    double q[WAGG_QUANT_MAX];
};

template <typename T> struct QuantKey;
template <> struct QuantKey<float> {
    typedef uint32_t U;
    static __device__ __forceinline__ U bits(float x) { return __float_as_uint(x); }
    static __device__ __forceinline__ float value(U u) { return __uint_as_float(u); }
};
template <> struct QuantKey<double> {
    typedef uint64_t U;
    static __device__ __forceinline__ U bits(double x) { return (U)__double_as_longlong(x); }
    static __device__ __forceinline__ double value(U u) { return __longlong_as_double((long long)u); }
};

// SEASON = false: doy / win are not read, every listed row counts.  Dynamic LDS: 128 * xf.max_rows bytes.
template <typename T, bool SEASON>
__global__ void __launch_bounds__(RL_BLOCK)
quantile_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
                const int32_t *__restrict__ doy, const int32_t *__restrict__ win, QuantXf xf, T *__restrict__ out, int64_t ldo,
                int64_t pstride, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    typedef typename QuantKey<T>::U U;
    constexpr int CELLS = 128 / (int)sizeof(T), SLOTS = RL_BLOCK / CELLS, BITS = 8 * (int)sizeof(T);
    constexpr U ONES = ~U(0), SIGN = U(1) << (BITS - 1);
    extern __shared__ __align__(16) unsigned char quantile_lds[];
    U *__restrict__ keys = reinterpret_cast<U *>(quantile_lds);       // [entry][cell]
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);                               // (cb: the tile; one part, one group: sg is 0)
    (void)sg;
    const int cell = (int)threadIdx.x % CELLS, slot = (int)threadIdx.x / CELLS;
    const int64_t col = (int64_t)cb * CELLS + cell;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, 0, b, e);
    const int32_t L = (int32_t)(e - b);                              // (n_rows < 2^31)
    if (L > xf.max_rows) {                                           // (block-uniform) the list does not fit the launch's LDS
        if (col < sh.n)
            for (int k = slot; k < xf.n_q; k += SLOTS) out[(int64_t)k * pstride + (int64_t)p * ldo + col] = (T)__builtin_nan("");
        if (threadIdx.x == 0) atomicOr(status, 2);
        return;
    }
    // ---- phase 1: the tile's column of keys
    int32_t w = 0;
    if constexpr (SEASON) w = col < sh.n ? win[col] : RL_WIN_NULL;
    bool saw_inf = false;
#pragma unroll 4
    for (int32_t i = slot; i < L; i += SLOTS) {
        const int64_t t = rows[b + i];
        const bool ok = t >= 0 && t < sh.T;                          // (a row index outside the field is never read)
        bool in = ok && col < sh.n;
        if constexpr (SEASON) {
            const int32_t d = ok ? doy[t] : -1;
            in = in && in_season(d, w);
        }
        U key = ONES;
        if (in) {
            const T x = X[t * sh.ldx + col];
            saw_inf |= (bool)__builtin_isinf(x);
            const U u = QuantKey<T>::bits(x);
            if (x == x) key = u ^ ((u & SIGN) != 0 ? ONES : SIGN);
        }
        keys[i * CELLS + cell] = key;
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
    __syncthreads();
    // ---- phase 2: exact selection in the cell's column
    if (col >= sh.n || slot >= xf.n_q) return;
    const U *__restrict__ column = keys + cell;
    int32_t m = 0;
#pragma unroll 8
    for (int32_t i = 0; i < L; ++i) m += column[i * CELLS] != ONES ? 1 : 0;
    for (int k = slot; k < xf.n_q; k += SLOTS) {
        T *o = out + (int64_t)k * pstride + (int64_t)p * ldo + col;
        if (m == 0) {
            *o = (T)__builtin_nan("");
            continue;
        }
        double qk = 0.0;
#pragma unroll
        for (int j = 0; j < WAGG_QUANT_MAX; ++j) qk = k == j ? xf.q[j] : qk;        // (xf.q is never indexed by a lane's value)
        const double h = (double)(m - 1) * qk;
        const int32_t lo = (int32_t)__builtin_floor(h);
        const double g = h - (double)lo;
        U key_lo = 0;
        int32_t r = lo;                                              // the rank wanted among the keys that agree with key_lo so far
        for (int bit = BITS - 1; bit >= 0; --bit) {
            int32_t c = 0;
#pragma unroll 8
            for (int32_t i = 0; i < L; ++i) c += ((column[i * CELLS] ^ key_lo) >> bit) == 0 ? 1 : 0;
            if (r >= c) {
                r -= c;
                key_lo |= U(1) << bit;
            }
        }
        U key_hi = key_lo;
        if (xf.method != WAGG_QUANT_LOWER && g != 0.0) {             // v[lo + 1]: a tie with v[lo], or the least key above it
            int32_t c_le = 0;
            U next = ONES;
#pragma unroll 8
            for (int32_t i = 0; i < L; ++i) {
                const U kk = column[i * CELLS];
                c_le += kk <= key_lo ? 1 : 0;
                next = kk > key_lo && kk < next ? kk : next;
            }
            if (lo + 1 >= c_le) key_hi = next;                       // (g != 0 puts lo + 1 below m: a valid key, never all-ones)
        }
        const double v_lo = (double)QuantKey<T>::value(key_lo ^ ((key_lo & SIGN) != 0 ? SIGN : ONES));
        const double v_hi = (double)QuantKey<T>::value(key_hi ^ ((key_hi & SIGN) != 0 ? SIGN : ONES));
        double res;
        if (xf.method == WAGG_QUANT_LINEAR) {
            const double d = v_hi - v_lo;
            const double step = d * g;
            res = g == 0.0 ? v_lo : v_lo + step;
        } else if (xf.method == WAGG_QUANT_LOWER) {
            res = v_lo;
        } else {
            res = g == 0.0 ? v_lo : v_hi;
        }
        *o = (T)(res + xf.offset);
    }
}

// flag |= 1 when a period's list (row_begin confined as the kernels confine it) holds more than max_rows entries
__global__ void quantile_longest_kernel(const int32_t *__restrict__ row_begin, int64_t P, int64_t n_rows, int32_t max_rows,
                                        int *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += stride) {
        int64_t b = row_begin[i], e = row_begin[i + 1];
        b = b < 0 ? 0 : (b > n_rows ? n_rows : b);
        e = e < b ? b : (e > n_rows ? n_rows : e);
        bad |= e - b > max_rows;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

static int quantile_check_longest(const int32_t *row_begin, int32_t P, int64_t n_rows, int32_t max_rows, hipStream_t st) {
    DevBuf<int> flag;                                                // (blocking, as rowlist_check_rows just was)
    int bad = 0;
    WAGG_HIP(flag.alloc(1));
    WAGG_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(quantile_longest_kernel, dim3(64), dim3(256), 0, st, row_begin, (int64_t)P, n_rows, max_rows, flag.p);
    WAGG_HIP(hipGetLastError());
    WAGG_HIP(staged_d2h(&bad, flag.p, sizeof(int), st));
    WAGG_REQUIRE(bad == 0, "row lists: a period lists more than max_rows = %d entries", (int)max_rows);
    return WAGG_OK;
}

// The host sequence is grouped_reduce's (wagg_rowlist.h), step for step and message for message, with what this family adds: the
// grid is tiles x periods (not 16-byte pieces), the launch carries dynamic LDS, and the look at the lists also bounds their length.
template <typename T>
static int quantile_select(const GroupedArgs<T> &a, double offset, const double *q, int n_q, int method, int32_t max_rows) {
    constexpr int CELLS = 128 / (int)sizeof(T);
    clear_error();
    WAGG_TRY(rowlist_require_sizes(a.Ttot, a.n, a.P, a.n_rows));
    WAGG_REQUIRE((a.flags & ~WAGG_PERIOD_ROWS_CHECKED) == 0, "unknown flags 0x%x (%s has no keep-NaN form)", a.flags, "a period quantile");
    WAGG_REQUIRE(n_q >= 1 && n_q <= WAGG_QUANT_MAX, "n_q must be 1..%d, got %d", WAGG_QUANT_MAX, n_q);
    WAGG_REQUIRE(q != nullptr, "q is NULL");
    for (int k = 0; k < n_q; ++k) WAGG_REQUIRE(q[k] >= 0.0 && q[k] <= 1.0, "quantile %d must lie in [0, 1], got %g", k, q[k]);
    WAGG_REQUIRE(method == WAGG_QUANT_LINEAR || method == WAGG_QUANT_LOWER || method == WAGG_QUANT_HIGHER,
                 "method must be WAGG_QUANT_LINEAR, WAGG_QUANT_LOWER or WAGG_QUANT_HIGHER, got %d", method);
    WAGG_REQUIRE(max_rows >= 1 && max_rows <= WAGG_QUANT_ROWS_MAX, "max_rows must be 1..%d, got %d", WAGG_QUANT_ROWS_MAX, (int)max_rows);
    WAGG_REQUIRE(std::isfinite(offset), "offset must be finite");
    WAGG_REQUIRE((a.doy == nullptr) == (a.win == nullptr), "doy_dev and win_dev go together: both given, or both NULL (no season)");
    WAGG_TRY(rowlist_require_layout(a.n, a.ldx, a.ldo, a.P, n_q, a.pstride, nullptr, 0, a.status, a.row_begin, a.rows, a.n_rows));
    if (a.P == 0 || a.n == 0) return WAGG_OK;
    WAGG_REQUIRE(a.out != nullptr, "NULL pointer (out_dev)");
    WAGG_REQUIRE(a.n_rows == 0 || a.Ttot == 0 || a.X != nullptr, "NULL pointer (%s)", "X_dev");
    const int64_t tiles = (a.n + CELLS - 1) / CELLS;
    WAGG_REQUIRE(tiles * (int64_t)a.P < (int64_t)0x7fffffff, "too many tiles x periods for one launch");
    hipStream_t st = (hipStream_t)a.stream;
    WAGG_TRY(rowlist_check_rows(a.row_begin, a.P, a.rows, a.n_rows, a.Ttot, a.flags, st));
    if (!(a.flags & WAGG_PERIOD_ROWS_CHECKED)) WAGG_TRY(quantile_check_longest(a.row_begin, a.P, a.n_rows, max_rows, st));
    RowlistShape sh;
    sh.T = a.Ttot; sh.n = a.n; sh.ldx = a.ldx; sh.n_rows = a.n_rows; sh.P = a.P;
    sh.n_colblk = (int32_t)tiles;
    sh.split = 1;
    sh.aux = 1;
    QuantXf xf = {};
    xf.n_q = n_q;
    xf.method = method;
    xf.max_rows = max_rows;
    xf.offset = offset;
    for (int k = 0; k < n_q; ++k) xf.q[k] = q[k];
    const size_t lds = (size_t)128 * (size_t)max_rows;
    const dim3 grid((unsigned)(tiles * a.P));
    auto go = [&](auto season) -> int {
        auto kern = quantile_kernel<T, decltype(season)::value>;
        WAGG_HIP(allow_dynamic_lds((const void *)kern, (size_t)128 * WAGG_QUANT_ROWS_MAX));      // (once a kernel: the most any call asks)
        hipLaunchKernelGGL(kern, grid, dim3(RL_BLOCK), lds, st, a.X, sh, a.row_begin, a.rows, a.doy, a.win, xf, a.out, a.ldo, a.pstride,
                           a.status);
        WAGG_HIP(hipGetLastError());
        return WAGG_OK;
    };
    return a.doy != nullptr ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace wagg

extern "C" int wagg_quantile_select_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                        const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                        double offset, const double *q, int n_q, int method, int32_t max_rows, int flags, float *out_dev,
                                        int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::quantile_select<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                         out_pstride, status_dev, nullptr, 0, stream}, offset, q, n_q, method, max_rows);
}
extern "C" int wagg_quantile_select_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                        const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                        double offset, const double *q, int n_q, int method, int32_t max_rows, int flags, double *out_dev,
                                        int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::quantile_select<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                          out_pstride, status_dev, nullptr, 0, stream}, offset, q, n_q, method, max_rows);
}
