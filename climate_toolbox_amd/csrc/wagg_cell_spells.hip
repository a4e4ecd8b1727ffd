// Spells and exceedances against PER-CELL thresholds (wagg_cell_spells_*): wagg_spells.hip's statistics with the threshold read
// from a field instead of a scalar register -- days above the cell's own 90th percentile (TX90p / TN10p), warm-spell days (WSDI /
// CSDI), events "above the local 95th percentile for 3 days", precipitation on days above the cell's 95th wet-day percentile
// (R95pTOT).  The consumer of what wagg_quantile_select_* leaves on the device.
//
// THE DEFINITION (include/wagg.h has the same text; tests/cell_spell_ref.py is its NumPy twin).  thr_dev is (n_thr, M, n) of the
// element type, thr[k][m][j] = thr_dev[k * thr_kstride + m * ldt + j].  A period p reads ONE plane m = plane_of_period[p] (NULL:
// m = 0 for M == 1, m = p for M == P).  Cell j, period p, threshold k: the entries i of rows[row_begin[p] : row_begin[p + 1]] are
// walked IN ORDER.  Entry i is HOT when t = rows[i] lies in [0, T), cell j is in season on doy[t] (when a season is given) and
// X[t, j] + offset >= thr[k][m][j] (below = 0) or < thr[k][m][j] (below = 1).  The comparison is the bins' exact rule, formed ON
// THE DEVICE: c = ceilT((double)thr - offset) -- one fp64 subtraction, rounded to nearest, stepped up once where that lies
// below, host ceil_to<T>'s rule -- and the hot test per row is x >= c / x < c on the RAW element, exactly the scalar kernel's.
// So a threshold field that is constant over the cells gives wagg_spell_reduce_*'s plane bit for bit.  +-inf thresholds compare
// as they compare.  A NaN THRESHOLD MAKES THAT CELL'S RESULT NaN for that threshold in that period, for every statistic.  Runs,
// gaps, seasons, NaN days and the status word are wagg_spells.hip's: a gap in the row numbers, an out-of-season day, a NaN and
// the end of the list end a run; RUNS ARE TRUNCATED AT PERIOD BOUNDARIES; a value out of season is selected away to NaN; a
// piece none of whose cells is in season is not read BUT STILL RESETS THE RUNS; an in-season +-inf sets bit 0 of the status word.
//   WAGG_SPELL_DAYS / _EVENTS / _LONGEST   as in wagg_spells.hip, int32 run and result per cell and threshold
//   WAGG_CELL_SPELL_AMOUNT   the sum over hot entries of  (double)x + offset
//   WAGG_CELL_SPELL_EXCESS   ... of  ((double)x + offset) - (double)thr   (below = 1:  (double)thr - ((double)x + offset))
// The two sums have an fp64 accumulator per cell and threshold and no run counter (min_length must be 1); each term is two
// separately rounded fp64 operations, the terms are added one by one IN LIST ORDER and the sum is cast once on the store.  The
// sequential order is the definition: a NumPy loop reproduces the bits.
//
// THE FRAME is spell_kernel's, copied (wagg_rowlist.h says why the row-list kernels do not share theirs): a lane owns one 16-byte
// piece of a row (VEC = 1 for unaligned rows), the grid is column block x period x group, one row in flight, strict list order,
// the wave-uniform gap test.  A LIST IS NEVER SPLIT and there is no workspace: work_dev / work_bytes are ignored.  What differs:
// the lane loads its group x VEC thresholds ONCE, ahead of the row loop, with load_piece -- a 16-byte load where the row is wide,
// so the wide route also asks that thr_dev be 16-byte aligned and ldt / thr_kstride be multiples of the piece (else VEC = 1) --
// and holds c[group][VEC] in vector registers where the scalar kernel holds thr[group] in scalar ones.  An out-of-range plane
// index (only reachable with WAGG_PERIOD_ROWS_CHECKED: the library's look at the lists rejects it otherwise) makes the block
// write NaN for its period and set status bit 2; it then reads no threshold at all.
//
// CS_G = WAGG_CELL_SPELL_GROUP = 4 thresholds a group.  hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage,
// VGPRs / scratch bytes / waves per SIMD, the greater of the season and no-season kernel of each family:
//                         fp32 VEC = 4     fp32 VEC = 1     fp64 VEC = 2     fp64 VEC = 1
//   days/events/longest   70 / 0 / 7      27 / 0 / 8      49 / 0 / 8      30 / 0 / 8
//   amount                72 / 0 / 7      28 / 0 / 8      51 / 0 / 8      32 / 0 / 8
//   excess                106 / 0 / 4     37 / 0 / 8      78 / 0 / 6      42 / 0 / 8
// No instance uses scratch, none spills an SGPR (at most 85), no AGPRs, no LDS.  Groups of 8 (the scalar kernel's) avoid scratch
// too, at fp32 VEC = 4 / fp64 VEC = 2:  counts 118 / 0 / 4 and 81 / 0 / 5,  amount 120 / 0 / 4 and 83 / 0 / 5,  excess 186 / 0 / 2 and
// 117 / 0 / 4 -- the scalar kernel's 86 plus the 32 thresholds it keeps in scalar registers.
// BOTH GROUP SIZES WERE TIMED through the public call at c2-real shape (tools/relative_timing.py; profiles/relative_timing.json,
// profiles/relative_timing_group8.json, the comparison in profiles/relative_timing_groups.json), at 3 levels and at 8 -- two groups
// of 4, one of 8: in none of 12 cases does either lead by the project's rule (a median ahead by more than the larger min - max
// spread).  With no faster one to keep, the group of 4 stays: the percentile triples this family is for (90 / 95 / 99) fit one
// group of 4 with one idle slot where a group of 8 computes five, and it holds fewer registers (more waves per SIMD).  The kernel
// alone (without the public call's host path) has not been timed.
//
// The host layer (CellSpellXf and its fill, cell_ceil_to, the argument checks, the pick of the STAT instance, the VEC = 1
// fallback of the threshold field, the blocking look's host sequence) is wagg_spell.h's, shared with wagg_cell_spells_rows.hip.
#include "wagg_spell.h"

namespace wagg {

constexpr int CS_G = WAGG_CELL_SPELL_GROUP;

// SEASON = false: doy / win are not read.  STAT: WAGG_SPELL_DAYS / _EVENTS / _LONGEST, WAGG_CELL_SPELL_AMOUNT / _EXCESS.
template <typename T, int VEC, bool SEASON, int STAT>
__global__ void __launch_bounds__(RL_BLOCK)
cell_spell_kernel(const T *__restrict__ X, RowlistShape sh, const int32_t *__restrict__ row_begin, const int32_t *__restrict__ rows,
                  const int32_t *__restrict__ doy, const int32_t *__restrict__ win, const T *__restrict__ thr_dev,
                  const int32_t *__restrict__ plane_of_period, CellSpellXf xf, T *__restrict__ out, int64_t ldo, int64_t pstride,
                  int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    constexpr bool SUM = STAT == WAGG_CELL_SPELL_AMOUNT || STAT == WAGG_CELL_SPELL_EXCESS;
    typedef std::conditional_t<SUM, double, int32_t> Acc;
    WAGG_ROWLIST_BLOCK(sh, cb, p, sg);
    const int32_t s = 0, k0 = (int32_t)sg * CS_G;                     // (one part: a list is never split)
    const int kg = xf.n_thr - k0 < CS_G ? xf.n_thr - k0 : CS_G;      // thresholds of this group (>= 1 by the grid's extent)
    const int64_t col = ((int64_t)cb * RL_BLOCK + threadIdx.x) * VEC;
    const int32_t m = plane_of_period != nullptr ? plane_of_period[p] : (xf.M == 1 ? 0 : p);       // (block-uniform)
    if (m < 0 || m >= xf.M) {                                        // no such plane: NaN for the period, and no threshold is read
        if (col < sh.n) {
            for (int k = 0; k < kg; ++k) {
                T *o = out + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
#pragma unroll
                for (int c = 0; c < VEC; ++c)
                    if (col + c < sh.n) o[c] = (T)__builtin_nan("");
            }
        }
        if (threadIdx.x == 0) atomicOr(status, 4);
        return;
    }
    WAGG_ROWLIST_ROWS(sh, row_begin, p, s, b, e);
    const int32_t L = xf.min_length;
    const bool below = xf.below != 0;
    const double off = xf.offset;
    bool saw_inf = false;
    if (col < sh.n) {
        T cmp[CS_G][VEC];                                            // ceilT((double)thr - offset): what the raw element is compared with
        [[maybe_unused]] T raw[CS_G][VEC];                           // the threshold itself (the excess subtracts it)
#pragma unroll
        for (int k = 0; k < CS_G; ++k) {                             // (a ragged group repeats its last threshold)
            const int64_t kk = k0 + k < xf.n_thr ? k0 + k : xf.n_thr - 1;
            T t[VEC];
            load_piece<T, VEC>(thr_dev + kk * xf.kstride + (int64_t)m * xf.ldt, col, sh.n, t);
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                cmp[k][c] = cell_ceil_to<T>((double)t[c] - off);
                if constexpr (STAT == WAGG_CELL_SPELL_EXCESS) raw[k][c] = t[c];
            }
        }
        [[maybe_unused]] int32_t run[CS_G][VEC];
        Acc acc[CS_G][VEC];
#pragma unroll
        for (int k = 0; k < CS_G; ++k)
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                if constexpr (!SUM) run[k][c] = 0;
                acc[k][c] = Acc(0);
            }
        int32_t w[VEC];                                              // the lane's windows, read once (cells past n: null)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if constexpr (SEASON) w[c] = col + c < sh.n ? win[col + c] : RL_WIN_NULL;
            else w[c] = 0;
        }
        int64_t prev = -2;                                           // the row of the entry before (no row follows -2)
        for (int64_t i = b; i < e; ++i) {
            const int64_t t = (int64_t)rows[i];
            const bool ok = t >= 0 && t < sh.T;                      // (wave-uniform; a row index outside the field is never read)
            const bool joins = t == prev + 1;                        // (wave-uniform: does this entry continue the one before?)
            prev = t;
            int32_t d = -1;
            if constexpr (SEASON) d = ok ? doy[t] : -1;              // (wave-uniform too: one scalar per row)
            T x[VEC];
            bool in[VEC], any = false;
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                if constexpr (SEASON) in[c] = in_season(d, w[c]);
                else in[c] = ok && col + c < sh.n;
                any |= in[c];
                x[c] = T(0);
            }
            if (any) load_piece<T, VEC>(X + t * sh.ldx, col, sh.n, x);      // no cell of this piece in season: no load
            if constexpr (!SUM) {
                if (!joins) {                                        // behind a gap in the row numbers every run starts anew
#pragma unroll
                    for (int k = 0; k < CS_G; ++k)
#pragma unroll
                        for (int c = 0; c < VEC; ++c) run[k][c] = 0;
                }
            }
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                saw_inf |= in[c] && __builtin_isinf(x[c]);
                const T v = in[c] ? x[c] : (T)__builtin_nan("");     // selected away: NaN is cold on either side
                [[maybe_unused]] const double a = (double)v + off;   // (the sums' first rounding)
#pragma unroll
                for (int k = 0; k < CS_G; ++k) {
                    const bool hot = below ? v < cmp[k][c] : v >= cmp[k][c];
                    if constexpr (SUM) {
                        double term = a;
                        if constexpr (STAT == WAGG_CELL_SPELL_EXCESS) term = below ? (double)raw[k][c] - a : a - (double)raw[k][c];
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
        for (int k = 0; k < CS_G; ++k) {
            if (k >= kg) continue;
            T *o = out + (int64_t)(k0 + k) * pstride + (int64_t)p * ldo + col;
#pragma unroll
            for (int c = 0; c < VEC; ++c)                            // (cmp is NaN exactly where the threshold is: offset is finite)
                if (col + c < sh.n) o[c] = cmp[k][c] != cmp[k][c] ? (T)__builtin_nan("") : (T)acc[k][c];
        }
    }
    if (__ballot(saw_inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

// flag |= 1 when a period's plane index lies outside [0, M)
__global__ void cell_spell_planes_kernel(const int32_t *__restrict__ plane_of_period, int64_t P, int32_t M, int *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += stride) {
        const int32_t m = plane_of_period[i];
        bad |= m < 0 || m >= M;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

template <typename T>
static int cell_spells(const GroupedArgs<T> &a, double offset, const T *thr_dev, int n_thr, int64_t ldt, int64_t kstride,
                       const int32_t *plane_of_period, int32_t M, int min_length, int stat, int below) {
    static const GroupedFamily fam = {"a per-cell spell count", "X_dev", 1, CS_G};
    int rc_planes = WAGG_OK;
    const int rc = grouped_reduce<T>(
        fam, a, n_thr,                                               // (not looked at unless n_thr passes the check)
        [&]() -> int {
            return cell_spell_require(n_thr, M, thr_dev, ldt, a.n, kstride, [&]() -> int {
                WAGG_REQUIRE(plane_of_period != nullptr || M == 1 || M == a.P,
                             "plane_of_period_dev is NULL: allowed only for M == 1 or M == P (M=%d, P=%d)", (int)M, (int)a.P);
                return WAGG_OK;
            }, offset, min_length, stat, below);
        },
        [&](const RowlistShape &got, bool wide, hipStream_t st) {
            if (plane_of_period != nullptr && !(a.flags & WAGG_PERIOD_ROWS_CHECKED)) {
                rc_planes = spell_flag_look(st, [&](int *flag) {
                    hipLaunchKernelGGL(cell_spell_planes_kernel, dim3(64), dim3(256), 0, st, plane_of_period, (int64_t)a.P, M, flag);
                }, "plane_of_period: every period's plane index must lie in [0, M = %d)", M);
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
                        hipLaunchKernelGGL((cell_spell_kernel<T, decltype(vec)::value, decltype(season)::value, decltype(stat_c)::value>),
                                           grid, dim3(RL_BLOCK), 0, st, a.X, sh, a.row_begin, a.rows, a.doy, a.win, thr_dev, plane_of_period,
                                           xf, out, ldo, pstride, a.status);
                    });
                }
            });
        });
    return rc != WAGG_OK ? rc : rc_planes;
}

}  // namespace wagg

extern "C" int wagg_cell_spells_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                    const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                    double offset, const float *thr_dev, int n_thr, int64_t ldt, int64_t thr_kstride,
                                    const int32_t *plane_of_period_dev, int32_t M, int min_length, int stat, int below, int flags,
                                    float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::cell_spells<float>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                     out_pstride, status_dev, nullptr, 0, stream}, offset, thr_dev, n_thr, ldt, thr_kstride,
                                    plane_of_period_dev, M, min_length, stat, below);
}
extern "C" int wagg_cell_spells_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                                    const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                                    double offset, const double *thr_dev, int n_thr, int64_t ldt, int64_t thr_kstride,
                                    const int32_t *plane_of_period_dev, int32_t M, int min_length, int stat, int below, int flags,
                                    double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *, int64_t, void *stream) {
    return wagg::cell_spells<double>({X_dev, nullptr, T, n, ldx, row_begin_dev, rows_dev, P, n_rows, doy_dev, win_dev, flags, out_dev, ldo,
                                      out_pstride, status_dev, nullptr, 0, stream}, offset, thr_dev, n_thr, ldt, thr_kstride,
                                     plane_of_period_dev, M, min_length, stat, below);
}
