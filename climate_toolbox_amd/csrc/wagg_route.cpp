// The route of a segment-table apply (wagg_route.h).  Plain C++: no HIP header, nothing allocated.
#include "wagg_route.h"

namespace wagg {

const char *route_refusal_text(int refuse) {
    return refuse == REFUSE_COMPACT_CHUNKING    ? "compact rows need the whole-line chunking of this plan and data type"
           : refuse == REFUSE_COMPACT_NOT_WHOLE ? "compact rows: the whole-line kernel did not take the whole plan"
                                                : "";
}

// ---- which kernel runs what (the only copy of this table; tests/golden/routes.json pins it case by case) -------------------
// Single-chunk ("normal") groups of a plan, by (element type, data layout, transform):
//   transform            (time, gridcell) data                          (gridcell, time) data
//   none / one power     sparse_lcv_kernel<T,VEC,1>      [L32 | L64]    sparse_lcv_kernel<T,VEC,1,false,GT>    [R | L64]
//   powers p..p+n-1 <= 4 sparse_lcv_kernel<T,VEC,n>      [L32 | L64]    sparse_lcv_kernel<T,VEC,n,false,GT>    [R | L64]
//   degree days, k <= 4  sparse_lcv_kernel<T,VEC,k,EDD>  [L64 | L64e]   sparse_lcv_kernel<T,VEC,k,EDD,GT>      [L64 | L64e]
// chunking in brackets, fp32 | fp64: R = region-shaped (<= 64 quads), L32 / L64 = eight whole 128-byte lines of 32 / 16
// cells, L64e = four lines of 16 cells (both fp64 fields of a chunk in one image row).  Where the chunking named does not
// exist (WAGG_PLAN_NO_LINES, a grid without a row length, a scattered table) or a WAGG_PLAN_NO_* flag says so: fp32 plain /
// powers stay on sparse_lcv_kernel with R; everything else takes sparse_stream_kernel (no transform, one power per pass) or
// the chunk-walking sparse_gather_kernel (degree days, (gridcell, time) data), which also serves every giant group.
// More than four powers / thresholds: several passes.
//
// sparse_lcv_kernel fuses up to four planes (powers or degree-day thresholds) in both element types and both layouts on the
// chunkings of the table; everything it does not serve (giant groups, plans whose flags or table shape rule its chunkings out)
// runs once per power with the transform applied on load.
SparseRoute sparse_route(const RoutePlan &p, const RouteCall &c) {
    SparseRoute r;
    const bool f32 = c.elem == 4, tg = c.layout == WAGG_LAYOUT_TG, edd = c.xf.kind == RX_EDD;
    const int nfuse = c.xf.kind == RX_POWERS ? c.xf.count : 1, n_thr = edd ? c.xf.count : 0;
    const bool lcv_off = route_lcv_off(p.flags);
    // degree days in sparse_lcv_kernel: fp32 fields on the 128-cell chunking (the fp64 one: 64-byte pieces)
    const bool edd_lcv = edd && route_lcv_lines(p, c.elem, true) != CH_R && n_thr >= 1 && n_thr <= 4;
    const bool use_lines = (edd_lcv && tg) || (route_lines_chunking(p, c.elem, false) != CH_R && tg && !edd && (nfuse == 1 || (nfuse <= 4 && !lcv_off)));
    // (gridcell, time) data in sparse_lcv_kernel: every cell of a chunk is fetched by itself (64 timesteps = two or four whole
    // lines), so fp32 takes the region-shaped chunks (fewest cells); fp64 the 128-cell whole-line chunking (a region-shaped
    // chunk holds 256)
    const bool gt_lcv = c.layout == WAGG_LAYOUT_GT && !lcv_off && (!edd || edd_lcv) && nfuse <= 4 && (f32 || p.has_lines64);
    r.chunking = edd_lcv ? (f32 ? CH_L64 : CH_L64E) : gt_lcv ? (f32 ? CH_R : CH_L64) : use_lines ? (f32 ? CH_L32 : CH_L64) : CH_R;
    const RouteChunking &d = p.ch[r.chunking];
    const int64_t Gcomp = c.compact == COMPACT_QUADS ? d.Gq : d.Gc;
    if (c.compact && !(use_lines && !lcv_off && nfuse <= 4 && (!edd || edd_lcv) && Gcomp > 0 && c.ldx >= Gcomp)) {
        r.refuse = REFUSE_COMPACT_CHUNKING;
        return r;
    }
    const int n_norm = (int)d.n_groups - d.g0_normal;
    if (nfuse > 1) {
        // fused: fp32 in either loader/consumer kernel; fp64 in sparse_lcv_kernel on its whole-line chunking
        const bool lc_ok = ((tg && (f32 || (use_lines && !lcv_off))) || gt_lcv) && !(p.flags & (WAGG_PLAN_NO_STREAM | WAGG_PLAN_NO_LC)) &&
                           n_norm > 0 && c.Ttot > 0;
        if (!lc_ok || nfuse > 4) {
            RouteCall one = c;
            one.xf.count = 1;
            r = sparse_route(p, one);
            r.per_power = true;
            return r;
        }
    }
    r.nplanes = edd ? (n_thr > 0 ? n_thr : 1) : nfuse;      // powers of the fused tas_poly, or thresholds of one degree-day pass
    if (c.Ttot == 0) return r;
    // (T x R) results: the kernels write region-major into a stream-ordered workspace, then one transpose; (R x T) results go
    // straight to the caller's buffer.  Whole-line chunkings: the kernels write PARTIAL rows (one per (chunk, region) entry)
    // into the workspace whatever the output layout; combine_parts_kernel sums a region's rows, divides and transposes
    const bool lines = d.n_part > 0;
    r.via_ws = (c.out_layout == WAGG_OUT_TR || lines) && d.n_groups > 0;
    r.ws_rows = lines ? d.n_part : p.R;
    // sparse_stream_kernel and sparse_gather_kernel fetch a quad as FOUR elements in one load: 32 bytes of a fp64 row, whose
    // 16-byte alignment says nothing about G % 4.  With ldx == G and G % 4 == 2 the region-shaped chunking's last quad
    // (cells G - 2, G - 1) would be read two elements past the end of the last row: such grids take the clamped arm.
    // (fp32: aligned rows have ldx % 4 == 0, so a quad never leaves its row.  sparse_lcv_kernel loads 16-byte pieces.)
    const bool vec_quad = c.aligned16 && (f32 || p.G % 4 == 0);
    // degree days (two fields): fp32 (time, gridcell) data in a loader/consumer kernel, everything else in the chunk-walking one
    const bool stream_path = (tg || gt_lcv) && !(p.flags & WAGG_PLAN_NO_STREAM) && (!edd || f32 || edd_lcv);
    if (stream_path && n_norm > 0) {
        // loaders + vector-ALU consumers: fp32 on either chunking, fp64 on its whole-line chunking only (a region-shaped chunk
        // of 64 quads is 2 KiB of a fp64 row: twice the image row)
        if (!(p.flags & (WAGG_PLAN_NO_LC | WAGG_PLAN_LC_MFMA)) && (!edd || edd_lcv) && nfuse <= 4 && (f32 || lines)) {
            r.main = MAIN_LCV; r.vec = c.aligned16; r.edd = edd_lcv; r.gt = gt_lcv; r.planes = edd_lcv ? r.nplanes : nfuse;
        } else if (f32 && (p.flags & WAGG_PLAN_LC_MFMA) && !(p.flags & WAGG_PLAN_NO_LC)) {
            r.main = MAIN_LC_MFMA; r.vec = c.aligned16;         // (diagnostic build, wagg_sparse_diag.hip)
        } else if (!edd) {
            r.main = MAIN_STREAM; r.vec = vec_quad;             // persistent pipelined kernel
        }
    }
    r.gather_groups = r.main != MAIN_NONE ? d.g0_normal : (int)d.n_groups;      // a main kernel leaves the giant groups
    r.gather_vec = tg && vec_quad;
    r.gather_nthr = edd && r.nplanes > 1 ? 4 : 1;
    if (c.compact && !(r.main != MAIN_NONE && r.gather_groups == 0)) r.refuse = REFUSE_COMPACT_NOT_WHOLE;
    // all planes of partial rows in one combine (regions without rows come out as 0 / den there); else per plane
    r.finish = r.via_ws && lines ? FIN_COMBINE : (r.via_ws ? FIN_TRANSPOSE : 0) | (d.n_empty > 0 ? FIN_FILL : 0);
    return r;
}

}  // namespace wagg
