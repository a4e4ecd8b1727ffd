// Which kernels one apply of a segment-table plan runs, decided once from a handful of plan scalars and call parameters.
// Plain C++ -- no HIP, no plan object, no allocation, O(1): launch_sparse (wagg_sparse.hip) fills the inputs, asks
// sparse_route and launches what the answer says; tests/route_dump.cpp links this unit alone and enumerates it.
#pragma once
#include <cstdint>

#include "../../include/wagg.h"

namespace wagg {

// the chunkings of a plan (wagg_plan: d, dl, dl64, dl64e): R = region-shaped (<= 64 quads), L32 / L64 = eight whole 128-byte
// lines of 32 / 16 cells, L64E = four lines of 16 cells (both fp64 fields of a chunk in one image row)
enum { CH_R = 0, CH_L32 = 1, CH_L64 = 2, CH_L64E = 3 };
constexpr int COMPACT_NONE = 0, COMPACT_LINES = 1, COMPACT_QUADS = 2;       // which row launch_sparse is handed

struct RouteChunking { int64_t n_groups = 0; int g0_normal = 0; int64_t n_part = 0, n_empty = 0, Gc = 0, Gq = 0; };
struct RoutePlan {
    int flags = 0;                                      // WAGG_PLAN_*
    bool has_lines = false, has_lines64 = false, has_lines64e = false;
    int64_t G = 0, R = 0;
    RouteChunking ch[4];                                // by CH_*
};

// the element transform of a call: none, powers first .. first + count - 1 of (x + offset), degree days at `count` thresholds
enum { RX_NONE = 0, RX_POWERS = 1, RX_EDD = 2 };
struct RouteTransform { int kind = RX_NONE, first = 0, count = 1; };
struct RouteCall {
    int elem = 4;                                       // bytes of an element
    int layout = WAGG_LAYOUT_TG, out_layout = WAGG_OUT_TR;
    RouteTransform xf;
    int compact = COMPACT_NONE;
    int64_t ldx = 0;
    bool aligned16 = false;                             // X (degree days: and X2) and the row pitch are 16-byte aligned
    int64_t Ttot = 0;
};

enum { MAIN_NONE = 0, MAIN_LCV = 1, MAIN_LC_MFMA = 2, MAIN_STREAM = 3 };
enum { FIN_FILL = 1, FIN_TRANSPOSE = 2, FIN_COMBINE = 4 };                  // bits of SparseRoute::finish
enum { REFUSE_NONE = 0, REFUSE_COMPACT_CHUNKING = 1, REFUSE_COMPACT_NOT_WHOLE = 2 };

struct SparseRoute {
    int refuse = REFUSE_NONE;   // REFUSE_COMPACT_CHUNKING: nothing runs; REFUSE_COMPACT_NOT_WHOLE: reported after the main kernel
    int chunking = CH_R;        // the chunking every kernel of the call reads
    bool per_power = false;     // fused powers the fused kernels do not take: the rest of the route is that of ONE power, run
                                // once per power (plane i at out + i * pstride)
    int main = MAIN_NONE;       // the kernel over the single-chunk groups
    bool vec = false;           // MAIN_LCV / MAIN_LC_MFMA: 16-byte loads; MAIN_STREAM: whole-quad loads
    bool edd = false, gt = false;   // MAIN_LCV: degree days, (gridcell, time) data
    int planes = 1;             // MAIN_LCV: fused powers or thresholds of the pass
    int gather_groups = 0;      // groups left for sparse_gather_kernel (all of them without a main kernel), once per power
    bool gather_vec = false;    // ... its whole-quad loads
    int gather_nthr = 1;        // ... its NTHR instance: 1, or 4 for more than one threshold
    int nplanes = 1;            // output planes of a pass
    bool via_ws = false;        // the kernels write region-major / partial rows into the plan's staging buffer
    int64_t ws_rows = 0;        // ... of this many rows per plane
    int finish = 0;             // FIN_COMBINE alone, or FIN_TRANSPOSE and / or FIN_FILL per plane
};

// sparse_lcv_kernel and the whole-line chunkings are ruled out by the plan's flags
inline bool route_lcv_off(int flags) { return (flags & (WAGG_PLAN_NO_LC | WAGG_PLAN_NO_STREAM | WAGG_PLAN_LC_MFMA)) != 0; }
// the whole-line chunking the plan holds for (time, gridcell) data of `elem` bytes -- plain / powers, or degree days (chunks
// whose two fields fill one 64 KiB image); CH_R: none
inline int route_lines_chunking(const RoutePlan &p, int elem, bool edd) {
    if (edd) return elem == 4 ? (p.has_lines64 ? CH_L64 : CH_R) : (p.has_lines64e ? CH_L64E : CH_R);
    return elem == 4 ? (p.has_lines ? CH_L32 : CH_R) : (p.has_lines64 ? CH_L64 : CH_R);
}
// ... where the plan's flags let sparse_lcv_kernel read it: what the compact rows of the host paths and of wagg_pack.hip are
// packed for, and what a many-plan fuses its weightings on
inline int route_lcv_lines(const RoutePlan &p, int elem, bool edd) { return route_lcv_off(p.flags) ? CH_R : route_lines_chunking(p, elem, edd); }

SparseRoute sparse_route(const RoutePlan &p, const RouteCall &c);
const char *route_refusal_text(int refuse);

}  // namespace wagg
