// The quads-only compact row (wagg_sparse_int.h: ucell_q, run_src_q / run_len_q, Gq) as a matrix of its own: what the
// lines-only host path ships per block and hands straight to its kernel, laid down as a (T, Gq) device matrix so that the
// row-list reductions (wagg_period.hip, wagg_season.hip, wagg_edd_ladder.hip) can sum it over time with n = Gq before the
// compact apply (WAGG_APPLY_COMPACT_ROWS) contracts the few rows that are left.
//   wagg_plan_compact_info / _cells   the row described: its width and the source cell of every position
//   wagg_pack_rows_*                  device-resident field(s) -> packed rows: pack_rows_kernel below
//   wagg_pack_rows_host_*             host-resident field(s) -> packed rows: the gather pipeline of wagg_host.hip in its
//                                     "no result" mode, every arrived block copied device to device into its rows
#include "wagg_sparse_int.h"

namespace wagg {
namespace {

constexpr int PK_THREADS = 256;   // pieces of a packed row per workgroup
constexpr int PK_ROWS = 16;       // rows per workgroup: the quad table is read once for all of them
constexpr int PK_UNROLL = 4;      // rows whose loads are in flight together

// the chunking whose quads-only map serves element type `elem_bytes` (nullptr: the plan has none)
const SparsePlanDev *compact_chunking(const wagg_plan *plan, int elem_bytes) {
    if (plan->is_many()) return nullptr;
    const int ch = route_lcv_lines(route_plan(plan), elem_bytes, false);       // (WAGG_PLAN_NO_LINES: the plan holds none)
    const SparsePlanDev &d = chunking_of(plan, ch);
    if (ch == CH_R || d.Gq <= 0 || d.run_len_q.empty() || d.n_groups - d.g0_normal <= 0 || d.g0_normal != 0) return nullptr;
    return &d;
}

// out[t][p] = piece p of the packed row of row t.  A piece is 16 bytes: E = 4 fp32 / 2 fp64 cells, so a quad is one piece
// (fp32) or two (fp64); with two fields the pieces of field 1 follow those of field 0.  Lane = piece: consecutive lanes write
// consecutive 16 bytes of a packed row and read runs of adjacent quads of the source row.  Block b of the flat grid owns piece
// block b % n_pblk of row block b / n_pblk (neighbouring workgroups walk the same source rows).
// VEC: every base address and pitch is 16-byte aligned -> one 16-byte load and store per piece; else element by element.
template <typename T, bool VEC>
__global__ __launch_bounds__(PK_THREADS) void pack_rows_kernel(const T *__restrict__ X, const T *__restrict__ X2, int64_t Tn, int64_t ldx,
                                                               const int32_t *__restrict__ quad_cell, int64_t n_pieces, int n_fields,
                                                               T *__restrict__ out, int64_t ldo, int64_t n_pblk) {
    constexpr int E = 16 / (int)sizeof(T);      // cells per piece
    constexpr int PPQ = 4 / E;                  // pieces per quad
    typedef T vec_t __attribute__((ext_vector_type(E)));
    const int64_t pb = (int64_t)blockIdx.x % n_pblk, rb = (int64_t)blockIdx.x / n_pblk;
    const int64_t p = pb * PK_THREADS + threadIdx.x;
    if (p >= n_pieces * n_fields) return;
    const int f = p >= n_pieces ? 1 : 0;
    const int64_t q = p - (int64_t)f * n_pieces;
    const int64_t cell = (int64_t)quad_cell[q / PPQ] + (q % PPQ) * E;
    const T *__restrict__ src = (f ? X2 : X) + cell;
    T *__restrict__ dst = out + p * E;
    const int64_t r0 = rb * PK_ROWS, r1 = r0 + PK_ROWS < Tn ? r0 + PK_ROWS : Tn;
    for (int64_t r = r0; r < r1; r += PK_UNROLL) {
        vec_t v[PK_UNROLL];
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            if (r + u < r1) {
                const T *s = src + (r + u) * ldx;
                if constexpr (VEC) {
                    v[u] = *reinterpret_cast<const vec_t *>(s);
                } else {
#pragma unroll
                    for (int c = 0; c < E; ++c) v[u][c] = s[c];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            if (r + u < r1) {
                T *o = dst + (r + u) * ldo;
                if constexpr (VEC) {
                    *reinterpret_cast<vec_t *>(o) = v[u];
                } else {
#pragma unroll
                    for (int c = 0; c < E; ++c) o[c] = v[u][c];
                }
            }
        }
    }
}

// the device quad table of `d` (the chunking of element type T), built on first use
template <typename T>
int quad_table(const wagg_plan *plan, const SparsePlanDev &d, const int32_t **table) {
    const int w = sizeof(T) == 4 ? 0 : 1;
    std::lock_guard<std::mutex> lock(plan->pack_mu);
    if (!plan->pack_ready[w]) {
        std::vector<int32_t> qc;
        qc.reserve((size_t)(d.Gq / 4));
        for (size_t k = 0; k < d.run_src_q.size(); ++k)
            for (int32_t c = 0; c < d.run_len_q[k]; c += 4) qc.push_back((int32_t)(d.run_src_q[k] + c));
        WAGG_REQUIRE((int64_t)qc.size() * 4 == d.Gq, "the quad runs of the plan do not add up to its compact row");
        WAGG_HIP(plan->pack_quads[w].upload(qc));
        WAGG_HIP(hipStreamSynchronize(nullptr));         // (once per plan: the table is then there for every stream)
        plan->pack_ready[w] = true;
    }
    *table = plan->pack_quads[w].p;
    return WAGG_OK;
}

int unsupported(const char *what, int elem_bytes) {
    set_error("%s: the plan has no quads-only compact row for %d-byte elements (a single segment-table plan with the whole-line "
              "chunking of that element type has one)", what, elem_bytes);
    return WAGG_EUNSUPPORTED;
}

template <typename T>
int check_pack_args(const wagg_plan *plan, const void *X, int64_t Tn, int64_t ldx, const void *out, int64_t ldo, int n_fields, int64_t Gq) {
    WAGG_REQUIRE(Tn >= 0, "T < 0");
    if (Tn == 0) return WAGG_OK;
    WAGG_REQUIRE(X != nullptr && out != nullptr, "X/out is NULL");
    WAGG_REQUIRE(ldx >= plan->info.G, "ldx %lld too small", (long long)ldx);
    WAGG_REQUIRE(ldo >= n_fields * Gq, "ldo %lld too small for %d field(s) of %lld packed cells", (long long)ldo, n_fields, (long long)Gq);
    int cur = 0;
    WAGG_HIP(hipGetDevice(&cur));
    WAGG_REQUIRE(cur == plan->device, "the plan was created on device %d, the current device is %d", plan->device, cur);
    return WAGG_OK;
}

template <typename T>
int pack_rows(const wagg_plan *plan, const T *X, const T *X2, int64_t Tn, int64_t ldx, T *out, int64_t ldo, hipStream_t stream) {
    WAGG_REQUIRE(plan != nullptr, "plan is NULL");
    const SparsePlanDev *d = compact_chunking(plan, (int)sizeof(T));
    if (!d) return unsupported("wagg_pack_rows", (int)sizeof(T));
    const int nf = X2 ? 2 : 1;
    if (int rc = check_pack_args<T>(plan, X, Tn, ldx, out, ldo, nf, d->Gq)) return rc;
    if (Tn == 0) return WAGG_OK;
    const int32_t *table = nullptr;
    if (int rc = quad_table<T>(plan, *d, &table)) return rc;
    const int64_t n_pieces = d->Gq * (int64_t)sizeof(T) / 16;
    const int64_t n_pblk = (n_pieces * nf + PK_THREADS - 1) / PK_THREADS, n_rblk = (Tn + PK_ROWS - 1) / PK_ROWS;
    WAGG_REQUIRE(n_pblk * n_rblk < (int64_t)0x7fffffff, "grid too large: %lld", (long long)(n_pblk * n_rblk));
    auto aligned = [](const void *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0; };
    const bool vec = aligned(X, ldx) && (!X2 || aligned(X2, ldx)) && aligned(out, ldo);
    auto kern = vec ? pack_rows_kernel<T, true> : pack_rows_kernel<T, false>;
    launch_timed(true, kern, dim3((unsigned)(n_pblk * n_rblk)), dim3(PK_THREADS), 0, stream, X, X2, Tn, ldx, table, n_pieces, nf, out, ldo, n_pblk);
    WAGG_HIP(hipGetLastError());
    return WAGG_OK;
}

// Host-resident field(s): the gather of the lines-only host path (wagg_host.hip), under the conditions of host_rows_pipeline
// (wagg_sparse.hip) for its quads-only rows.  WAGG_EUNSUPPORTED, with nothing queued, when it cannot be had.
template <typename T>
int pack_rows_host(const wagg_plan *plan, const T *X, const T *X2, int64_t Tn, int64_t ldx, T *out, int64_t ldo, int flags) {
    clear_error();
    WAGG_REQUIRE(plan != nullptr, "plan is NULL");
    WAGG_REQUIRE((flags & ~WAGG_HOST_PIN) == 0, "unknown host flags 0x%x", flags);
    const SparsePlanDev *d = compact_chunking(plan, (int)sizeof(T));
    if (!d) return unsupported("wagg_pack_rows_host", (int)sizeof(T));
    const int nf = X2 ? 2 : 1;
    const int64_t Gq = d->Gq, G = plan->info.G;
    if (int rc = check_pack_args<T>(plan, X, Tn, ldx, out, ldo, nf, Gq)) return rc;
    if (Tn == 0) return WAGG_OK;
    if (!(5 * Gq <= 4 * G && Tn * G * (int64_t)sizeof(T) >= ((int64_t)64 << 20) && gather_team_threads() >= 10)) {
        set_error("wagg_pack_rows_host: the gather is not worth it here (packed row %lld of %lld cells, field of %lld bytes, %d packing "
                  "threads)", (long long)Gq, (long long)G, (long long)(Tn * G * (int64_t)sizeof(T)), gather_team_threads());
        return WAGG_EUNSUPPORTED;
    }
    std::vector<int64_t> src(d->run_src_q.size());
    std::vector<int32_t> len(d->run_len_q.size());
    for (size_t k = 0; k < src.size(); ++k) { src[k] = d->run_src_q[k] * (int64_t)sizeof(T); len[k] = d->run_len_q[k] * (int32_t)sizeof(T); }
    HostRowsArgs a;
    a.X_host = reinterpret_cast<const char *>(X); a.X2_host = reinterpret_cast<const char *>(X2); a.out_host = nullptr;
    a.Tn = Tn;
    a.ldx_bytes = ldx * (int64_t)sizeof(T); a.xrow_bytes = G * (int64_t)sizeof(T);
    a.ldo_bytes = 0; a.orow_bytes = 0;
    a.quantum = 64; a.flags = 0; a.n_dev = 1; a.devices = nullptr;
    a.run_src = src.data(); a.run_len = len.data(); a.n_runs = (int64_t)src.size(); a.crow_bytes = Gq * (int64_t)sizeof(T);
    a.no_result = true;
    const size_t brow = (size_t)(nf * Gq) * sizeof(T);   // bytes of a packed row as the blocks arrive (field 0, then field 1)
    int64_t next_row = 0;                                 // (one device: the blocks arrive in row order)
    a.apply = [&](int, const void *xd, int64_t rows, void *, hipStream_t st) -> int {
        WAGG_HIP(hipMemcpy2DAsync(out + next_row * ldo, (size_t)ldo * sizeof(T), xd, brow, brow, (size_t)rows, hipMemcpyDeviceToDevice, st));
        next_row += rows;
        return WAGG_OK;
    };
    return stream_host_rows_any(a);
}

}  // namespace
}  // namespace wagg

extern "C" int wagg_plan_compact_info(const wagg_plan *plan, int elem_bytes, int64_t *Gq) {
    WAGG_REQUIRE(plan != nullptr && Gq != nullptr, "NULL argument");
    WAGG_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 or 8, got %d", elem_bytes);
    const wagg::SparsePlanDev *d = wagg::compact_chunking(plan, elem_bytes);
    *Gq = d ? d->Gq : 0;
    return WAGG_OK;
}

extern "C" int wagg_plan_compact_cells(const wagg_plan *plan, int elem_bytes, int32_t *cell_of_pos_host) {
    WAGG_REQUIRE(plan != nullptr && cell_of_pos_host != nullptr, "NULL argument");
    WAGG_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 or 8, got %d", elem_bytes);
    const wagg::SparsePlanDev *d = wagg::compact_chunking(plan, elem_bytes);
    if (!d) return wagg::unsupported("wagg_plan_compact_cells", elem_bytes);
    int64_t pos = 0;
    for (size_t k = 0; k < d->run_src_q.size(); ++k)
        for (int32_t c = 0; c < d->run_len_q[k]; ++c) cell_of_pos_host[pos++] = (int32_t)(d->run_src_q[k] + c);
    WAGG_REQUIRE(pos == d->Gq, "the quad runs of the plan do not add up to its compact row");
    return WAGG_OK;
}

extern "C" int wagg_pack_rows_f32(const wagg_plan *plan, const float *X_dev, const float *X2_dev, int64_t T, int64_t ldx, float *out_dev,
                                  int64_t ldo, void *stream) {
    return wagg::pack_rows<float>(plan, X_dev, X2_dev, T, ldx, out_dev, ldo, (hipStream_t)stream);
}
extern "C" int wagg_pack_rows_f64(const wagg_plan *plan, const double *X_dev, const double *X2_dev, int64_t T, int64_t ldx, double *out_dev,
                                  int64_t ldo, void *stream) {
    return wagg::pack_rows<double>(plan, X_dev, X2_dev, T, ldx, out_dev, ldo, (hipStream_t)stream);
}
extern "C" int wagg_pack_rows_host_f32(const wagg_plan *plan, const float *X_host, const float *X2_host, int64_t T, int64_t ldx,
                                       float *out_dev, int64_t ldo, int flags) {
    return wagg::pack_rows_host<float>(plan, X_host, X2_host, T, ldx, out_dev, ldo, flags);
}
extern "C" int wagg_pack_rows_host_f64(const wagg_plan *plan, const double *X_host, const double *X2_host, int64_t T, int64_t ldx,
                                       double *out_dev, int64_t ldo, int flags) {
    return wagg::pack_rows_host<double>(plan, X_host, X2_host, T, ldx, out_dev, ldo, flags);
}
