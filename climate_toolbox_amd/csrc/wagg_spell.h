// What the four spell units hold in common on the HOST (wagg_spells.hip, wagg_spells_span.hip, wagg_cell_spells.hip,
// wagg_cell_spells_rows.hip): the transform structs their kernels take and how they are filled, the argument checks of a spell
// call in the one order all of them have always had, the pick of the STAT instance, the VEC = 1 fallback of a threshold field
// and the blocking "flag kernel" look at plane indices.  The two pairs: SCALAR thresholds (spell_reduce, spell_span: a list of
// doubles on the host) and PER-CELL thresholds (cell_spells, cell_spells_rows: a (n_thr, M, n) field on the device).  A unit
// keeps its kernel, its GroupedFamily, a launch lambda of a few lines and its extern "C" twins.
// The kernel bodies stay copies, as wagg_rowlist.h says of the row-list kernels: behind shared inline functions hipcc allocates
// other registers (docs/HISTORY.md, "one shared core"), and these kernels sit at occupancy edges.  The one device function here,
// cell_ceil_to, was already __forceinline__ with one body under two names.
#pragma once
#include "wagg_rowlist.h"

#include <cmath>

namespace wagg {

// ---- scalar thresholds ---------------------------------------------------------------------------------------------------------
template <typename T> struct SpellXf {
    int n_thr, min_length, below;
    T c[WAGG_SPELL_MAX];                        // ceilT(thresholds[k] - offset)
};

template <typename T> inline SpellXf<T> spell_xf(const double *thresholds, int n_thr, double offset, int min_length, int below) {
    SpellXf<T> xf;
    xf.n_thr = n_thr;
    xf.min_length = min_length;
    xf.below = below;
    for (int k = 0; k < WAGG_SPELL_MAX; ++k) xf.c[k] = ceil_to<T>(thresholds[k < n_thr ? k : n_thr - 1] - offset);
    return xf;
}

// ---- per-cell thresholds -------------------------------------------------------------------------------------------------------
struct CellSpellXf {
    int n_thr, min_length, below;
    int32_t M;
    double offset;
    int64_t ldt, kstride;
};

inline CellSpellXf cell_spell_xf(int n_thr, int64_t ldt, int64_t kstride, int32_t M, double offset, int min_length, int below) {
    CellSpellXf xf;
    xf.n_thr = n_thr;
    xf.min_length = min_length;
    xf.below = below;
    xf.M = M;
    xf.offset = offset;
    xf.ldt = ldt;
    xf.kstride = kstride;
    return xf;
}

// host ceil_to<T> on the device: the smallest value of T that is not below c (NaN stays NaN)
template <typename T> __device__ __forceinline__ T cell_ceil_to(double c) {
    if constexpr (sizeof(T) == 8) {
        return c;
    } else {
        float f = (float)c;                                          // (to nearest; +-inf and what overflows stay / become +-inf)
        if ((double)f < c) {                                         // one step towards +inf, as nextafterf takes it
            const uint32_t u = __float_as_uint(f);
            f = f == 0.0f ? __uint_as_float(1u) : __uint_as_float((u >> 31) != 0 ? u - 1u : u + 1u);      // (-inf steps to -FLT_MAX)
        }
        return f;
    }
}

// ---- the checks of a spell call's own parameter list (grouped_reduce's check()); each returns WAGG_OK or sets the error text
// and returns the code.  A head per pair, then the tail all four share.
inline bool spell_is_sum(int stat) { return stat == WAGG_CELL_SPELL_AMOUNT || stat == WAGG_CELL_SPELL_EXCESS; }

// min_length, stat, the rules of single statistics, below.  sums: the two fp64 sums are statistics of this call (the per-cell pair)
inline int spell_require_tail(int min_length, int stat, int below, bool sums) {
    WAGG_REQUIRE(min_length >= 1 && min_length <= WAGG_SPELL_MIN_LENGTH_MAX, "min_length must be 1..%d, got %d",
                 WAGG_SPELL_MIN_LENGTH_MAX, min_length);
    const bool counts = stat == WAGG_SPELL_DAYS || stat == WAGG_SPELL_EVENTS || stat == WAGG_SPELL_LONGEST;
    if (sums) {
        WAGG_REQUIRE(counts || spell_is_sum(stat),
                     "stat must be WAGG_SPELL_DAYS, _EVENTS, _LONGEST or WAGG_CELL_SPELL_AMOUNT, _EXCESS, got %d", stat);
    } else {
        WAGG_REQUIRE(counts, "stat must be WAGG_SPELL_DAYS, _EVENTS or _LONGEST, got %d", stat);
    }
    WAGG_REQUIRE(stat != WAGG_SPELL_LONGEST || min_length == 1, "WAGG_SPELL_LONGEST does not use min_length: it must be 1, got %d",
                 min_length);
    WAGG_REQUIRE(!spell_is_sum(stat) || min_length == 1,
                 "WAGG_CELL_SPELL_AMOUNT / _EXCESS have no run counter: min_length must be 1, got %d", min_length);
    WAGG_REQUIRE(below == 0 || below == 1, "below must be 0 or 1, got %d", below);
    return WAGG_OK;
}

inline int spell_require(int n_thr, const double *thresholds, double offset, int min_length, int stat, int below) {
    WAGG_REQUIRE(n_thr >= 1 && n_thr <= WAGG_SPELL_MAX, "n_thr must be 1..%d, got %d", WAGG_SPELL_MAX, n_thr);
    WAGG_REQUIRE(thresholds != nullptr, "thresholds is NULL");
    WAGG_REQUIRE(std::isfinite(offset), "offset must be finite");
    for (int k = 0; k < n_thr; ++k) {
        WAGG_REQUIRE(thresholds[k] == thresholds[k], "threshold %d is NaN", k);
        WAGG_REQUIRE(!std::isinf(thresholds[k]), "threshold %d is infinite (a constant plane)", k);
    }
    return spell_require_tail(min_length, stat, below, false);
}

// plane(): what the family asks of its plane map's pointer -- its own requirement, at the place it has always had
template <typename Plane>
inline int cell_spell_require(int n_thr, int32_t M, const void *thr_dev, int64_t ldt, int64_t n, int64_t kstride, Plane &&plane,
                              double offset, int min_length, int stat, int below) {
    WAGG_REQUIRE(n_thr >= 1 && n_thr <= WAGG_CELL_SPELL_MAX, "n_thr must be 1..%d, got %d", WAGG_CELL_SPELL_MAX, n_thr);
    WAGG_REQUIRE(M >= 1, "M must be at least 1, got %d", (int)M);
    WAGG_REQUIRE(thr_dev != nullptr, "thr_dev is NULL");
    WAGG_REQUIRE(ldt >= n, "ldt smaller than n (ldt=%lld, n=%lld)", (long long)ldt, (long long)n);
    WAGG_REQUIRE(ldt <= INT64_MAX / M && kstride >= (int64_t)M * ldt, "thr_kstride smaller than M * ldt");
    WAGG_TRY(plane());
    WAGG_REQUIRE(std::isfinite(offset), "offset must be finite");
    return spell_require_tail(min_length, stat, below, true);
}

// ---- the launch ----------------------------------------------------------------------------------------------------------------
// go(std::integral_constant<int, STAT>{}) for the call's statistic.  SUMS = false (the scalar pair, whose check has rejected the
// two sums) instantiates no kernel for them.
template <bool SUMS, typename Go> inline void spell_with_stat(int stat, Go &&go) {
    if (stat == WAGG_SPELL_DAYS) go(std::integral_constant<int, WAGG_SPELL_DAYS>{});
    else if (stat == WAGG_SPELL_EVENTS) go(std::integral_constant<int, WAGG_SPELL_EVENTS>{});
    else if (!SUMS || stat == WAGG_SPELL_LONGEST) go(std::integral_constant<int, WAGG_SPELL_LONGEST>{});
    else if constexpr (SUMS) {
        if (stat == WAGG_CELL_SPELL_AMOUNT) go(std::integral_constant<int, WAGG_CELL_SPELL_AMOUNT>{});
        else go(std::integral_constant<int, WAGG_CELL_SPELL_EXCESS>{});
    }
}

// The wide route reads a lane's thresholds with load_piece too, so it also asks that thr_dev be 16-byte aligned and ldt /
// kstride be multiples of the piece; where they are not: VEC = 1 for field and thresholds, with the column blocks of that route.
// False: those are too many blocks for one launch (the error text is set).
template <typename T>
inline bool cell_spell_narrow(RowlistShape &sh, bool &wide, const T *thr_dev, int n_thr, int64_t ldt, int64_t kstride, int32_t M) {
    constexpr int V = 16 / (int)sizeof(T);
    if (!wide || ((reinterpret_cast<uintptr_t>(thr_dev) & 15) == 0 && (M == 1 || ldt % V == 0) && (n_thr == 1 || kstride % V == 0)))
        return true;
    wide = false;                                                    // the thresholds cannot be read in 16-byte pieces: VEC = 1 for both
    sh.n_colblk = (int32_t)((sh.n + RL_BLOCK - 1) / RL_BLOCK);
    if ((int64_t)sh.n_colblk * sh.P * sh.aux >= (int64_t)0x7fffffff) {
        set_error("too many pieces x periods x groups for one launch");
        return false;
    }
    return true;
}

// One blocking look through a kernel that ORs 1 into a flag word where it finds fault: launch(flag) starts the family's kernel
// on st; msg (with M for its %d) is the error when the flag came back set.
template <typename Launch> inline int spell_flag_look(hipStream_t st, Launch &&launch, const char *msg, int32_t M) {
    DevBuf<int> flag;                                                // (blocking, as rowlist_check_rows just was)
    int bad = 0;
    WAGG_HIP(flag.alloc(1));
    WAGG_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    launch(flag.p);
    WAGG_HIP(hipGetLastError());
    WAGG_HIP(staged_d2h(&bad, flag.p, sizeof(int), st));
    WAGG_REQUIRE(bad == 0, msg, (int)M);
    return WAGG_OK;
}

}  // namespace wagg
