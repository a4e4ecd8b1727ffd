// What the row-list reductions hold in common (wagg_period.hip, wagg_season.hip, wagg_edd_ladder.hip, wagg_bins.hip,
// wagg_hinge.hip, wagg_exposure.hip): a lane owns one 16-byte piece of a row (VEC = 1 for rows that are not 16-byte aligned)
// and walks its period's row list; the grid is column block x period x part [x group of thresholds / bins / knots], flat; when
// that cannot fill the device a period's list is cut into `split` consecutive parts, every part writes fp64 partial sums to the
// caller's workspace [s][plane][p][j] and rowlist_finish adds them in part order -- no atomics on a sum. The five families
// before the exposure bins promise each other bit equality (an all-year season = the period sum, every ladder plane = the
// four-plane kernels' plane, a one-knot hinge call = the plane of the many-knot call, counts that do not depend on the split):
// that rests on the split rule, the part arithmetic and the finish order being the ones below for all of them.  The host pieces
// are defined once, in wagg_period.hip; the four grouped families (ladder, bins, hinge, exposure) also share their whole host
// sequence, grouped_reduce below.  The frame of their kernel bodies (window read, rows in flight, masks, loads, status word)
// deliberately stays a copy in each: behind shared inline functions hipcc allocates other registers (docs/HISTORY.md, "one
// shared core").
#pragma once
#include "wagg_common.h"

#include <cmath>
#include <type_traits>

namespace wagg {

constexpr int RL_BLOCK = 256;
constexpr int RL_TARGET_BLOCKS = 1024;      // 256 CUs x 4: below this a period's rows are split
constexpr int RL_MAX_SPLIT = 64;
constexpr int RL_MIN_ROWS_PER_PART = 8;
constexpr int RL_NONE = 0, RL_POLY = 1, RL_EDD = 2;               // MODE of the four-plane kernels
constexpr int RL_MAX_PLANES = 4;
constexpr int32_t RL_WIN_NULL = 1 << 21, RL_WIN_INVERT = 1 << 20;  // include/wagg.h: bits 0-9 first day, 10-19 last day

struct RowlistShape {
    int64_t T, n, ldx, n_rows;
    int32_t P, n_colblk, split;
    int32_t aux;                            // period: keep_nan; season: 0; grouped families: the number of groups
};

template <typename T> struct RowlistXf {    // the four-plane kernels' transform
    T off;
    int pow_first, planes;
    T thr[RL_MAX_PLANES];
};

// is day-of-year d inside the packed window w?  (a null window and a day outside 0..1023 are in no season)
__device__ __forceinline__ bool in_season(int32_t d, int32_t w) {
    const int32_t a = w & 1023, b = (w >> 10) & 1023;
    const bool inside = d >= a && d <= b;
    return (w & RL_WIN_NULL) == 0 && (uint32_t)d <= 1023u && inside != ((w & RL_WIN_INVERT) != 0);
}

// the cells [col, col + VEC) of one row; a piece that would reach past n is read cell by cell (cells past n read 0)
template <typename T, int VEC>
__device__ __forceinline__ void load_piece(const T *__restrict__ row, int64_t col, int64_t n, T (&v)[VEC]) {
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

// What blockIdx.x stands for, and the rows of `rows` a block sums.  Two macros that declare the caller's variables, not inline
// functions: hipcc allocates the reduce kernels' registers by the order of these statements among the kernel's own (the
// same statements behind an inlined call, or the second group ahead of `col`, renames registers and moves tens of
// instructions in most instances), and the kernels are to stay the code whose registers and timings are on record.
//   WAGG_ROWLIST_BLOCK: column block cb, period p, and sg = the part s of p's list (grouped families: s + split * group)
//   WAGG_ROWLIST_ROWS:  [b, e) = part s of period p's list; a malformed row_begin is confined to the list's extent
#define WAGG_ROWLIST_BLOCK(sh, cb, p, sg)                                                     \
    const int64_t blk_ = blockIdx.x;                                                          \
    const int32_t cb = (int32_t)(blk_ % (sh).n_colblk);                                       \
    const int64_t ps_ = blk_ / (sh).n_colblk;                                                 \
    const int32_t p = (int32_t)(ps_ % (sh).P);                                                \
    const int64_t sg = ps_ / (sh).P
#define WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e)                                          \
    int64_t b = (row_begin)[p], e = (row_begin)[(p) + 1];                                     \
    b = b < 0 ? 0 : (b > (sh).n_rows ? (sh).n_rows : b);                                      \
    e = e < b ? b : (e > (sh).n_rows ? (sh).n_rows : e);                                      \
    if ((sh).split > 1) {                                                                     \
        const int64_t part_ = (e - b + (sh).split - 1) / (sh).split;                          \
        b = b + part_ * (s) < e ? b + part_ * (s) : e;                                        \
        e = b + part_ < e ? b + part_ : e;                                                    \
    }

#define WAGG_TRY(expr)                                                                        \
    do {                                                                                      \
        const int rc__ = (expr);                                                              \
        if (rc__ != WAGG_OK) return rc__;                                                     \
    } while (0)

// ---- host side; each returns WAGG_OK or sets the error text and returns the code ------------------------------------------
// the plane limits of a four-plane call (transform is one of WAGG_XF_NONE / _POLY / _EDD) and its transform as the kernels take it
template <typename T>
inline int rowlist_xf(int transform, double offset, int pow_first, int n_pow, const double *thresholds, int n_thr, RowlistXf<T> &xf) {
    xf.planes = 1;
    if (transform == WAGG_XF_POLY) {
        WAGG_REQUIRE(n_pow >= 1 && n_pow <= RL_MAX_PLANES && pow_first >= 1 && pow_first + n_pow - 1 <= 16,
                     "n_pow must be 1..%d and the powers 1..16 (pow_first=%d, n_pow=%d)", RL_MAX_PLANES, pow_first, n_pow);
        xf.planes = n_pow;
    } else if (transform == WAGG_XF_EDD) {
        WAGG_REQUIRE(n_thr >= 1 && n_thr <= RL_MAX_PLANES, "n_thr must be 1..%d, got %d", RL_MAX_PLANES, n_thr);
        WAGG_REQUIRE(thresholds != nullptr, "thresholds is NULL");
        xf.planes = n_thr;
    }
    xf.off = (T)offset;
    xf.pow_first = pow_first;
    for (int k = 0; k < RL_MAX_PLANES; ++k) xf.thr[k] = (T)(transform == WAGG_XF_EDD && k < n_thr ? thresholds[k] : 0.0);
    return WAGG_OK;
}

// the smallest value of T that is not below c (c is not NaN): the exact comparison of the bins and the spells, x >= ceil_to<T>(c)
// for a value x of T exactly when (double)x >= c
template <typename T> inline T ceil_to(double c) {
    if constexpr (sizeof(T) == 8) {
        return c;
    } else {
        float f = (float)c;                                          // (to nearest; +-inf and what overflows stay / become +-inf)
        if ((double)f < c) f = std::nextafterf(f, HUGE_VALF);         // (-inf for c < -FLT_MAX steps to -FLT_MAX >= c)
        return f;
    }
}

// The checks every entry point makes, in the order it has always made them: the sizes first, then -- behind the entry point's
// own checks of transform, planes and flags -- strides, workspace and the pointers that must be there even for an empty call.
int rowlist_require_sizes(int64_t T, int64_t n, int32_t P, int64_t n_rows);
int rowlist_require_layout(int64_t n, int64_t ldx, int64_t ldo, int32_t P, int planes, int64_t pstride, const void *work,
                           int64_t work_bytes, const void *status, const void *row_begin, const void *rows, int64_t n_rows);
// one blocking look at the lists unless flags has WAGG_PERIOD_ROWS_CHECKED: row_begin ascends within [0, n_rows], rows lie in [0, T)
int rowlist_check_rows(const int32_t *row_begin, int32_t P, const int32_t *rows, int64_t n_rows, int64_t T, int flags, hipStream_t st);

// how many consecutive parts a period's row list is cut into so that the grid fills the device.  Threshold groups do not
// enter: they multiply the blocks, but the parts decide the order of the fp64 additions.
int rowlist_split(int64_t n, int64_t P, int64_t n_rows, int vec);
int64_t rowlist_work_bytes(int64_t n, int64_t P, int64_t n_rows, int planes);       // behind the grouped families' *_work_bytes

// sh.T .. sh.P and sh.aux are the caller's; fills sh.n_colblk and sh.split (the rule's, cut to what `work` holds) and says
// whether rows are read in 16-byte pieces (X2 = NULL: one field).  False: n_colblk x P x split x n_grp is too many blocks.
bool rowlist_geometry(RowlistShape &sh, bool &wide, int elem_bytes, const void *X, const void *X2, int planes, const void *work,
                      int64_t work_bytes, int n_grp = 1);

// out[k][p][j] = (T) sum_s work[s][k][p][j], s ascending; nothing to do for split <= 1
template <typename T>
int rowlist_finish(const double *work, int split, int planes, int64_t P, int64_t n, T *out, int64_t ldo, int64_t pstride, hipStream_t st);

// ---- the grouped families (wagg_edd_ladder.hip, wagg_bins.hip, wagg_hinge.hip, wagg_exposure.hip) ---------------------------
// what their entry points take alike (X2: the ladder's and the exposure bins' tasmax; NULL in the one-field families)
template <typename T> struct GroupedArgs {
    const T *X, *X2;
    int64_t Ttot, n, ldx;
    const int32_t *row_begin, *rows;
    int32_t P;
    int64_t n_rows;
    const int32_t *doy, *win;
    int flags;
    T *out;
    int64_t ldo, pstride;
    int32_t *status;
    void *work;
    int64_t work_bytes;
    void *stream;
};

// what tells them apart outside their callbacks: the noun of the flags message, the field pointers a call that reads rows needs
// and their names in the message, the planes one block of the group dimension serves
struct GroupedFamily {
    const char *noun, *fields;
    int n_fields, group;
};

// The host sequence of a grouped entry point, in the one order all of them have always had.  check(): the family's checks of its
// own parameter list (WAGG_OK, or the error set and its code); planes: the planes of `out`, read only behind check();
// launch(sh, wide, st): builds the family's transform and launches through grouped_launch.
template <typename T, typename Check, typename Launch>
int grouped_reduce(const GroupedFamily &fam, const GroupedArgs<T> &a, int planes, Check &&check, Launch &&launch) {
    clear_error();
    WAGG_TRY(rowlist_require_sizes(a.Ttot, a.n, a.P, a.n_rows));
    WAGG_REQUIRE((a.flags & ~WAGG_PERIOD_ROWS_CHECKED) == 0, "unknown flags 0x%x (%s has no keep-NaN form)", a.flags, fam.noun);
    WAGG_TRY(check());
    WAGG_REQUIRE((a.doy == nullptr) == (a.win == nullptr), "doy_dev and win_dev go together: both given, or both NULL (no season)");
    WAGG_TRY(rowlist_require_layout(a.n, a.ldx, a.ldo, a.P, planes, a.pstride, a.work, a.work_bytes, a.status, a.row_begin, a.rows,
                                    a.n_rows));
    if (a.P == 0 || a.n == 0) return WAGG_OK;
    WAGG_REQUIRE(a.out != nullptr, "NULL pointer (out_dev)");
    WAGG_REQUIRE(a.n_rows == 0 || a.Ttot == 0 || (a.X != nullptr && (fam.n_fields < 2 || a.X2 != nullptr)), "NULL pointer (%s)",
                 fam.fields);
    hipStream_t st = (hipStream_t)a.stream;
    WAGG_TRY(rowlist_check_rows(a.row_begin, a.P, a.rows, a.n_rows, a.Ttot, a.flags, st));
    RowlistShape sh;
    sh.T = a.Ttot; sh.n = a.n; sh.ldx = a.ldx; sh.n_rows = a.n_rows; sh.P = a.P;
    sh.aux = (planes + fam.group - 1) / fam.group;
    bool wide;
    WAGG_REQUIRE(rowlist_geometry(sh, wide, (int)sizeof(T), a.X, a.X2, planes, a.work, a.work_bytes, sh.aux),
                 "too many pieces x periods x groups for one launch");
    launch(sh, wide, st);
    WAGG_HIP(hipGetLastError());
    return rowlist_finish<T>(static_cast<double *>(a.work), sh.split, planes, a.P, a.n, a.out, a.ldo, a.pstride, st);
}

// The kernel instance of one grouped launch and its grid (column block x period x part x group): VEC = a 16-byte piece of the
// row (wide) or 1, SEASON = doy given, DST = double with the workspace's strides (n, P * n) when the lists are split, else T
// with the caller's.  go(vec, season, grid, dst, ldo, pstride) launches <T, vec.value, season.value, ..., *dst's type>; what
// else picks an instance (the hinge's TAIL) is go's own business.
template <typename T, typename Go>
void grouped_launch(const RowlistShape &sh, bool wide, const GroupedArgs<T> &a, Go &&go) {
    const dim3 grid((unsigned)((int64_t)sh.n_colblk * sh.P * sh.split * sh.aux));
    auto with_dst = [&](auto vec, auto season) {
        if (sh.split > 1) go(vec, season, grid, static_cast<double *>(a.work), sh.n, (int64_t)sh.P * sh.n);
        else go(vec, season, grid, a.out, a.ldo, a.pstride);
    };
    auto with_season = [&](auto vec) {
        if (a.doy != nullptr) with_dst(vec, std::true_type{});
        else with_dst(vec, std::false_type{});
    };
    if (wide) with_season(std::integral_constant<int, 16 / (int)sizeof(T)>{});
    else with_season(std::integral_constant<int, 1>{});
}

}  // namespace wagg
