// Spells and exceedances against per-cell thresholds that change FROM ROW TO ROW (wagg_row_cell_spells_*): wagg_cell_spells.hip's
// statistics with the threshold plane picked per ENTRY of a period's list instead of per period -- calendar-day percentiles inside an
// annual period, ETCCDI's TX90p / TN10p / WSDI / CSDI as published (each day against the percentile of its own calendar day).
// (The entry points are named wagg_row_cell_spells_*, not wagg_cell_spells_rows_*: the wagg_cell_* names of the binding list are
// the by-period family's alone, which tests/test_cell_spell_host.py holds to.)
//
// THE DEFINITION (include/wagg.h has the same text; tests/cell_spell_rows_ref.py is its NumPy twin).  thr_dev is (n_thr, M, n) of the
// element type, thr[k][m][j] = thr_dev[k * thr_kstride + m * ldt + j].  Cell j, period p, threshold k: the entries i of
// rows[row_begin[p] : row_begin[p + 1]] are walked IN ORDER.  Entry i, with row t = rows[i] in [0, T), reads plane m =
// plane_of_row[t] (wave-uniform: one scalar per row, as doy[t] is).  Entry i is HOT when t lies in [0, T), cell j is in season on
// doy[t] (when a season is given) and X[t, j] + offset >= thr[k][m][j] (below = 0) or < thr[k][m][j] (below = 1).  The comparison is
// the bins' exact rule, formed ON THE DEVICE PER ROW: c = ceilT((double)thr[k][m][j] - offset) -- one fp64 subtraction, rounded to
// nearest, stepped up once where that lies below, cell_ceil_to<T> of wagg_spell.h -- and the hot test is x >= c / x < c on
// the RAW element.  With offset == 0, c is the threshold itself, and the kernel takes it without the arithmetic (a block-uniform
// branch: ceilT((double)thr - 0) is thr, bit for bit).  +-inf thresholds compare as they compare.  Runs, gaps, seasons, NaN days
// and bit 0 of the status word are wagg_cell_spells.hip's: a gap in the row numbers, an out-of-season day, a NaN and the end of the
// list end a run; RUNS ARE TRUNCATED AT PERIOD BOUNDARIES; a value out of season is selected away to NaN; a piece none of whose
// cells is in season loads NEITHER the field NOR a threshold BUT STILL RESETS THE RUNS; an in-season +-inf sets bit 0.
//   WAGG_SPELL_DAYS / _EVENTS / _LONGEST   as in wagg_spells.hip, int32 run and result per cell and threshold
//   WAGG_CELL_SPELL_AMOUNT   the sum over hot entries of  (double)x + offset
//   WAGG_CELL_SPELL_EXCESS   ... of  ((double)x + offset) - (double)thr   (below = 1:  (double)thr - ((double)x + offset)), thr being
//                            the raw threshold OF THAT ROW
// The two sums are sequential fp64 sums in list order, cast once on the store (min_length must be 1).
// NaN THRESHOLDS: out[k][p][j] is NaN if any COUNTED entry of the period had a NaN threshold for that cell and level -- a counted
// entry being one whose row is in the field and on which the cell is in season.  A sticky bit per (level, lane cell), no second
// pass.  CONSEQUENCE: a cell with no counted entry in a period gives 0, where wagg_cell_spells_* writes NaN for a NaN threshold
// even then (it reads its one plane ahead of the rows; here a plane is read only with a counted row).
// PLANE INDICES: without WAGG_PERIOD_ROWS_CHECKED the library's blocking look also checks plane_of_row[rows[i]] in [0, M) for every
// listed entry whose row lies in the field (WAGG_EINVAL before any launch).  With the flag, a block that meets an out-of-range
// index reads no threshold for that row, and at the end writes NaN for its whole period and sets status bit 2.  Rows that no list
// names need no valid plane.
//
// THE FRAME is spell_kernel's, copied as the sibling copied it: a lane owns one 16-byte piece of a row (VEC = 1 for unaligned
// rows), the grid is column block x period x group, strict list order, the wave-uniform gap test; the wide-route
// conditions on thr_dev, ldt and thr_kstride are the sibling's too (wagg_spell.h holds them once).  A LIST IS NEVER SPLIT and there is no workspace.  What differs:
//   RAGGED GROUPS   kg, the levels a block owns, is block-uniform: the kernel branches on it once into a body instantiated for kg
//                   = 1 .. CSR_G, so a ragged group issues no load and does no arithmetic for a level it does not own (TX90p's
//                   single level: two 16-byte loads a row, not five).
//   LOADS IN FLIGHT a row's field piece and its kg threshold pieces are issued together, ahead of the first use: a row costs one
//                   memory latency, not 1 + kg.  The row's three scalars (rows[i], plane_of_row[t], doy[t]: a dependent chain
//                   of scalar loads) are fetched ONE ENTRY AHEAD, so the vector loads of a row do not wait for them.
//   NEXT ROW'S VECTOR LOADS ARE NOT PREFETCHED.  It would hold (1 + kg) x VEC more registers a lane (20 at fp32 VEC = 4, kg = 4)
//                   on top of the table below, where fp32 VEC = 4 already stands at 4 waves a SIMD; the waves of a SIMD cover
//                   the latency by taking turns.  A prefetching variant was not built and not timed: the decision rests on
//                   the register count, not on a measurement.
// MEMORY TRAFFIC: the kernel reads (1 + K) x the field's bytes -- every counted row reads its own piece of K planes.  A plane
// is re-read once per evaluated year; holding several years' run state per lane to reuse a plane is not built.
//
// CSR_G = WAGG_CELL_SPELL_GROUP = 4 thresholds a group (the sibling's; no other size was timed for this kernel).  hipcc -O3
// --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage, VGPRs / scratch bytes / waves per SIMD, the greater of the
// season and no-season kernel of each family (a kernel holds the bodies of all four kg, with and without an offset):
//                         fp32 VEC = 4     fp32 VEC = 1     fp64 VEC = 2     fp64 VEC = 1
//   days/events/longest   105 / 0 / 4     38 / 0 / 8      76 / 0 / 6      40 / 0 / 8
//   amount                108 / 0 / 4     38 / 0 / 8      76 / 0 / 6      40 / 0 / 8
//   excess                110 / 0 / 4     40 / 0 / 8      76 / 0 / 6      41 / 0 / 8
// No instance uses scratch, none spills an SGPR (at most 102), no AGPRs, no LDS.  fp32 VEC = 4 holds 30 to 40 registers more than
// the sibling (a row's thresholds beside its values, where the sibling keeps one converted set for the whole list).
//
// The host layer (CellSpellXf and its fill, cell_ceil_to, the argument checks, the pick of the STAT instance, the VEC = 1
// fallback of the threshold field, the blocking look's host sequence) is wagg_spell.h's, shared with wagg_cell_spells.hip.
#include "wagg_spell.h"

namespace wagg {

constexpr int CSR_G = WAGG_CELL_SPELL_GROUP;

// the row loop and the stores of a block that owns KG levels, k0 .. k0 + KG - 1 (col < sh.n); PLAIN: offset == 0, c is the threshold
// itself.  True: the lane saw an in-season +-inf
template <typename T, int VEC, bool SEASON, int STAT, int KG, bool PLAIN>
__device__ __forceinline__ bool cell_spell_rows_body(const T *__restrict__ X, const RowlistShape &sh, const int32_t *__restrict__ rows,
                                                     const int32_t *__restrict__ doy, const int32_t *__restrict__ win,
                                                     const T *__restrict__ thr_dev, const int32_t *__restrict__ plane_of_row,
                                                     const CellSpellXf &xf, T *__restrict__ out, int64_t ldo, int64_t pstride,
                                                     int32_t *__restrict__ status, int32_t p, int32_t k0, int64_t col, int64_t b, int64_t e) {
#pragma clang fp contract(off)
    constexpr bool SUM = STAT == WAGG_CELL_SPELL_AMOUNT || STAT == WAGG_CELL_SPELL_EXCESS;
    typedef std::conditional_t<SUM, double, int32_t> Acc;
    const int32_t L = xf.min_length;
    const bool below = xf.below != 0;
    const double off = xf.offset;
    bool saw_inf = false, bad_plane = false;
    uint32_t nan_thr = 0;                                            // bit k * VEC + c: a counted entry's threshold was NaN
    [[maybe_unused]] int32_t run[KG][VEC];
    Acc acc[KG][VEC];
#pragma unroll
    for (int k = 0; k < KG; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (!SUM) run[k][c] = 0;
            acc[k][c] = Acc(0);
        }
    int32_t w[VEC];                                                  // the lane's windows, read once (cells past n: null)
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
        if constexpr (SEASON) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
        else w[c] = 0;
    }
    const T *const thr_col = thr_dev + (int64_t)k0 * xf.kstride;
    [[maybe_unused]] const bool whole = col + VEC <= sh.n;           // the lane's piece lies inside the row: one 16-byte load
    // where the lane stores and which of its cells exist, formed ahead of the loop: two vector registers and one live across it
    // in place of the scalars they are made of (held to the end, those do not fit the scalar file at fp32 VEC = 4 with a season)
    T *const o0 = out + (int64_t)k0 * pstride + (int64_t)p * ldo + col;
    uint32_t cells = 0;
#pragma unroll
    for (int c = 0; c < VEC; ++c) cells |= col + c < sh.n ? 1u << c : 0u;
    int64_t prev = -2;                                               // the row of the entry before (no row follows -2)
    // an entry's scalars are there when its turn comes (all wave-uniform; a row index outside the field is never used as one):
    // the row number is fetched two entries ahead, its plane and day one entry ahead -- issued at the head of an iteration,
    // they travel beside that iteration's vector loads
    int64_t t_n = b < e ? (int64_t)rows[b] : -1, t_nn = b + 1 < e ? (int64_t)rows[b + 1] : -1;
    bool ok_n = t_n >= 0 && t_n < sh.T;
    int32_t m_n = ok_n ? plane_of_row[t_n] : 0, d_n = -1;
    if constexpr (SEASON) d_n = ok_n ? doy[t_n] : -1;
    for (int64_t i = b; i < e; ++i) {
        const int64_t t = t_n;
        const bool ok = ok_n;
        const int32_t m = m_n, d = d_n;
        const bool joins = t == prev + 1;                            // (wave-uniform: does this entry continue the one before?)
        prev = t;
        t_n = t_nn;                                                  // (-1 behind the list's end: nothing is fetched for it)
        ok_n = t_n >= 0 && t_n < sh.T;
        m_n = ok_n ? plane_of_row[t_n] : 0;
        if constexpr (SEASON) d_n = ok_n ? doy[t_n] : -1;
        t_nn = i + 2 < e ? (int64_t)rows[i + 2] : -1;
        const bool m_ok = m >= 0 && m < xf.M;                        // (wave-uniform; m is 0 for a row outside the field)
        bad_plane |= !m_ok;
        T x[VEC], th[KG][VEC];                                       // (th: 0 where the cell is not counted -- never NaN there, never hot)
        bool in[VEC], any = false;
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (SEASON) {
                // (the window is decoded anew for every row: hoisted out of the loop, its flags become a scalar register pair per
                // cell, which at fp32 VEC = 4 the scalar file does not hold beside the rest)
                asm volatile("" : "+v"(w[c]));
                in[c] = in_season(d, w[c]);
            } else {
                in[c] = ok && col + c < sh.n;
            }
            any |= in[c];
            x[c] = T(0);
        }
#pragma unroll
        for (int k = 0; k < KG; ++k)
#pragma unroll
            for (int c = 0; c < VEC; ++c) th[k][c] = T(0);
        if (any) {                                                   // no cell of this piece in season: no load, of either
            const T *const xrow = X + t * sh.ldx + col;              // the field's piece and the KG threshold pieces go out together
            const T *const plane = thr_col + (int64_t)(m_ok ? m : 0) * xf.ldt + col;      // (not read unless m_ok)
            if (VEC == 1 || whole) {
                typedef T vec_t __attribute__((ext_vector_type(VEC)));
                const vec_t xv = *reinterpret_cast<const vec_t *>(xrow);
                vec_t tv[KG];
                if (m_ok) {
#pragma unroll
                    for (int k = 0; k < KG; ++k) tv[k] = *reinterpret_cast<const vec_t *>(plane + (int64_t)k * xf.kstride);
                }
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    x[c] = xv[c];
                    if (m_ok) {
#pragma unroll
                        for (int k = 0; k < KG; ++k) th[k][c] = tv[k][c];
                    }
                }
            } else {                                                 // the piece that reaches past n: cell by cell (in[c] implies col + c < n)
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    if (in[c]) {
                        x[c] = xrow[c];
                        if (m_ok) {
#pragma unroll
                            for (int k = 0; k < KG; ++k) th[k][c] = plane[(int64_t)k * xf.kstride + c];
                        }
                    }
                }
            }
        }
        if constexpr (!SUM) {
            if (!joins) {                                            // behind a gap in the row numbers every run starts anew
#pragma unroll
                for (int k = 0; k < KG; ++k)
#pragma unroll
                    for (int c = 0; c < VEC; ++c) run[k][c] = 0;
            }
        }
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            const T v = in[c] ? x[c] : (T)__builtin_nan("");         // selected away: NaN is cold on either side
            saw_inf |= __builtin_isinf(v);
            [[maybe_unused]] const double a = (double)v + off;       // (the sums' first rounding)
#pragma unroll
            for (int k = 0; k < KG; ++k) {
                const T raw = in[c] ? th[k][c] : T(0);               // (a counted entry: in the field, in season)
                nan_thr |= raw != raw ? 1u << (k * VEC + c) : 0u;
                T cmp = raw;                                         // ceilT((double)thr - offset): what the raw element is compared with
                if constexpr (!PLAIN) cmp = cell_ceil_to<T>((double)raw - off);
                const bool hot = below ? v < cmp : v >= cmp;
                if constexpr (SUM) {
                    double term = a;
                    if constexpr (STAT == WAGG_CELL_SPELL_EXCESS) term = below ? (double)raw - a : a - (double)raw;
                    acc[k][c] = hot ? acc[k][c] + term : acc[k][c];
                } else {
                    const int32_t r = hot ? run[k][c] + 1 : 0;
                    run[k][c] = r;
                    if constexpr (STAT == WAGG_SPELL_DAYS) acc[k][c] += r == L ? L : (r > L ? 1 : 0);
                    else if constexpr (STAT == WAGG_SPELL_EVENTS) acc[k][c] += r == L ? 1 : 0;
                    else acc[k][c] = r > acc[k][c] ? r : acc[k][c];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        T *o = o0 + (int64_t)k * pstride;
#pragma unroll
        for (int c = 0; c < VEC; ++c)
            if ((cells >> c & 1u) != 0) o[c] = bad_plane || (nan_thr >> (k * VEC + c) & 1u) != 0 ? (T)__builtin_nan("") : (T)acc[k][c];
    }
    if (bad_plane && threadIdx.x == 0) atomicOr(status, 4);          // (block-uniform: every wave walks the same list)
    return saw_inf;
}

// SEASON = false: doy / win are not read.  STAT: WAGG_SPELL_DAYS / _EVENTS / _LONGEST, WAGG_CELL_SPELL_AMOUNT / _EXCESS.
template <typename T, int VEC, bool SEASON, int STAT>
__global__ void __launch_bounds__(RL_BLOCK)
cell_spell_rows_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
                       const int32_t *__restrict__ doy, const int32_t *__restrict__ win, const T *__restrict__ thr_dev,
                       const int32_t *__restrict__ plane_of_row, CellSpellXf xf, T *__restrict__ out, int64_t ldo, int64_t pstride,
                       int32_t *__restrict__ status) {
    static_assert(CSR_G == 4, "the dispatch below names the group sizes 1..4");
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = 0, k0 = (int32_t)sg * CSR_G;                    // (one part: a list is never split)
    const int kg = xf.n_thr - k0 < CSR_G ? xf.n_thr - k0 : CSR_G;     // thresholds of this group (>= 1 by the grid's extent; block-uniform)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    bool saw_inf = false;
    if (col < sh.n) {
#define WAGG_CSR_BODY(KG, PLAIN) cell_spell_rows_body<T, VEC, SEASON, STAT, KG, PLAIN>(X, sh, rows, doy, win, thr_dev, plane_of_row, xf, out, ldo, \
                                                                                      pstride, status, p, k0, col, b, e)
        if (xf.offset == 0.0) {                                      // (block-uniform, as kg is)
            if (kg == 1) saw_inf = WAGG_CSR_BODY(1, true);
            else if (kg == 2) saw_inf = WAGG_CSR_BODY(2, true);
            else if (kg == 3) saw_inf = WAGG_CSR_BODY(3, true);
            else saw_inf = WAGG_CSR_BODY(4, true);
        } else {
            if (kg == 1) saw_inf = WAGG_CSR_BODY(1, false);
            else if (kg == 2) saw_inf = WAGG_CSR_BODY(2, false);
            else if (kg == 3) saw_inf = WAGG_CSR_BODY(3, false);
            else saw_inf = WAGG_CSR_BODY(4, false);
        }
#undef WAGG_CSR_BODY
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

// flag |= 1 when a listed entry whose row lies in the field has a plane index outside [0, M)
__global__ void cell_spell_row_planes_kernel(const int32_t *__restrict__ row_begin, int32_t P, const int32_t *__restrict__ rows,
                                             int64_t n_rows, int64_t T, const int32_t *__restrict__ plane_of_row, int32_t M,
                                             int *__restrict__ flag) {
    int64_t b = row_begin[0], e = row_begin[P];                      // (the entries the lists name, confined to the list's extent)
    b = b < 0 ? 0 : (b > n_rows ? n_rows : b);
    e = e < b ? b : (e > n_rows ? n_rows : e);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += stride) {
        const int64_t t = rows[i];
        if (t >= 0 && t < T) {
            const int32_t m = plane_of_row[t];
            bad |= m < 0 || m >= M;
        }
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

template <typename T>
static int cell_spells_rows(const GroupedArgs<T> &a, double offset, const T *thr_dev, int n_thr, int64_t ldt, int64_t kstride,
                            const int32_t *plane_of_row, int32_t M, int min_length, int stat, int below) {
    static const GroupedFamily fam = {"a per-cell spell count", "X_dev", 1, CSR_G};
    int rc_planes = WAGG_OK;
    const int rc = grouped_reduce<T>(
        fam, a, n_thr,                                               // (not looked at unless n_thr passes the check)
        [&]() -> int {
            return cell_spell_require(n_thr, M, thr_dev, ldt, a.n, kstride, [&]() -> int {
                WAGG_REQUIRE(plane_of_row != nullptr, "plane_of_row_dev is NULL");
                return WAGG_OK;
            }, offset, min_length, stat, below);
        },
        [&](const RowlistShape &got, bool wide, hipStream_t st) {
            if (!(a.flags & WAGG_PERIOD_ROWS_CHECKED) && a.n_rows != 0) {
                rc_planes = spell_flag_look(st, [&](int *flag) {
                    hipLaunchKernelGGL(cell_spell_row_planes_kernel, dim3(64), dim3(256), 0, st, a.row_begin, a.P, a.rows, a.n_rows, a.Ttot,
                                       plane_of_row, M, flag);
                }, "plane_of_row: the plane index of every listed row must lie in [0, M = %d)", M);
                if (rc_planes != WAGG_OK) return;                    // (nothing is launched)
            }
            RowlistShape sh = got;
            sh.split = 1;                                            // (no workspace went in; a run does not add across parts)
            if (!cell_spell_narrow<T>(sh, wide, thr_dev, n_thr, ldt, kstride, M)) {
                rc_planes = WAGG_EINVAL;
                return;
            }
            const CellSpellXf xf = cell_spell_xf(n_thr, ldt, kstride, M, offset, min_length, below);
            grouped_launch<T>(sh, wide, a, [&](auto vec, auto season, dim3 grid, auto *out, int64_t ldo, int64_t pstride) {
                if constexpr (std::is_same_v<std::remove_pointer_t<decltype(out)>, T>) {      // (split = 1: never the workspace)
                    spell_with_stat<true>(stat, [&](auto stat_c) {
                        hipLaunchKernelGGL((cell_spell_rows_kernel<T, decltype(vec)::value, decltype(season)::value, decltype(stat_c)::value>),
                                           grid, dim3(RL_BLOCK), 0, st, a.X, sh, a.row_begin, a.rows, a.doy, a.win, thr_dev, plane_of_row,
                                           xf, out, ldo, pstride, a.status);
                    });
                }
            });
        });
    return rc != WAGG_OK ? rc : rc_planes;
}

}  // namespace wagg

extern "C" int wagg_row_cell_spells_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                         const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev,
                                         const int32_t *win_dev, double offset, const float *thr_dev, int n_thr, int64_t ldt,
                                         int64_t thr_kstride, const int32_t *plane_of_row_dev, int32_t M, int min_length, int stat,
                                         int below, int flags, float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev,
                                         void *, int64_t, void *stream) {
    return wagg::cell_spells_rows<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev,
                                          ldo, out_pstride, status_dev, nullptr, 0, stream}, offset, thr_dev, n_thr, ldt, thr_kstride,
                                         plane_of_row_dev, M, min_length, stat, below);
}
extern "C" int wagg_row_cell_spells_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                         const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev,
                                         const int32_t *win_dev, double offset, const double *thr_dev, int n_thr, int64_t ldt,
                                         int64_t thr_kstride, const int32_t *plane_of_row_dev, int32_t M, int min_length, int stat,
                                         int below, int flags, double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev,
                                         void *, int64_t, void *stream) {
    return wagg::cell_spells_rows<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags,
                                           out_dev, ldo, out_pstride, status_dev, nullptr, 0, stream}, offset, thr_dev, n_thr, ldt,
                                          thr_kstride, plane_of_row_dev, M, min_length, stat, below);
}
