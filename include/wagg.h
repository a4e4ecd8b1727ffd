/* wagg.h -- C-ABI of the MI355X (gfx950) weighted grid->region aggregation engine (libwagg.so).
 *
 * This is the drop-in boundary for ONE path of ClimateImpactLab/climate_toolbox:
 *
 *   climate_toolbox/aggregations/aggregations.py
 *     :8-32    _reindex_spatial_data_to_regions      (pointwise gather, live branch :24-27)
 *     :35-84   _aggregate_reindexed_data_to_regions  (backup fill :73, grouped sums :78-79, divide)
 *     :87-124  weighted_aggregate_grid_to_regions    (:121-122 = the two above)
 *
 * The reference has no FFI; these entry points are what a ctypes binding placed at
 * aggregations.py:121-122 would call (INTEGRATION.md shows that binding).  Everything the
 * reference does with float LABELS (exact lat/lon match :27, backup fill :73, sorted unique
 * region labels :78) is resolved on the host in fp64 -- by the caller or by the host-side entry
 * points wagg_resolve_cells / wagg_backup_fill / wagg_factorize_* below; what reaches the
 * device-side entry points is the coded segment table (cell_idx, region_code, w_eff) and plain
 * device/host pointers.  The helpers either side of the path that have been folded in
 * (tas_poly, snyder_edd: transformations.py) are evaluated while the data is loaded
 * (wagg_apply_poly_*, wagg_apply_edd_*).  Since round 6 every apply is ONE entry point, wagg_apply(const
 * wagg_apply_desc *) at the end of this header; the per-combination wagg_*apply* functions below are wrappers
 * around it and stay for existing bindings.
 *
 * Conventions: every function returns 0 (WAGG_OK) or a negative wagg_status; nothing throws,
 * nothing calls exit(); wagg_last_error() gives the thread-local message of the last failure.
 * Plans are immutable after creation: concurrent wagg_apply_* on distinct streams is allowed,
 * create/destroy must not race with apply.  "_dev" pointers are HIP device pointers on the
 * current device; stream is a hipStream_t passed as void* (NULL = the null stream).
 * wagg_apply_* on device pointers is asynchronous on `stream`; the *_host_* forms block.
 */
#ifndef WAGG_H
#define WAGG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum wagg_status {
    WAGG_OK = 0,
    WAGG_EINVAL = -1,  /* bad argument (shape, index out of range, null pointer) */
    WAGG_EHIP = -2,    /* a HIP runtime call failed; see wagg_last_error() */
    WAGG_ENOMEM = -3,  /* host or device allocation failed */
    WAGG_ENODEV = -4,  /* no gfx950 device visible */
    WAGG_EUNSUPPORTED = -5,
    WAGG_EKEY = -6,    /* a segment label is absent from the grid (the reference's KeyError, S1) */
    WAGG_EINTERNAL = -7 /* an exception other than bad_alloc inside the library (never crosses the C boundary) */
} wagg_status;

/* memory layout of the flattened data matrix X and of the result */
#define WAGG_LAYOUT_TG 0 /* X[t*ldx + g]  -- (time, lat, lon) files: gridcell axis contiguous   */
#define WAGG_LAYOUT_GT 1 /* X[g*ldx + t]  -- (lat, lon, time) test fixture: time axis contiguous */
#define WAGG_OUT_TR 0    /* out[t*ldo + r]  (S10: (time, region)) */
#define WAGG_OUT_RT 1    /* out[r*ldo + t]  (S10 for the fixture layout: (region, time)) */

typedef struct wagg_plan wagg_plan;   /* sparse: coded segment table, region-grouped gather form */
typedef struct wagg_dense wagg_dense; /* dense (gridcell x region) fp32 weight matrix in HBM      */

typedef struct wagg_plan_info {
    int64_t nseg_in;     /* rows handed to wagg_plan_create                                      */
    int64_t nnz;         /* coalesced (cell, region) pairs kept (null label / NaN weight dropped) */
    int64_t n_groups;    /* region groups (one workgroup walks one group per time block)        */
    int64_t n_chunks;    /* LDS gather chunks (<= 256 unique cells each)                         */
    int64_t n_ucells;    /* sum over chunks of unique cells gathered per timestep                */
    int64_t n_giant;     /* regions with more unique cells than one chunk                       */
    int64_t n_empty;     /* regions with no kept segment (result 0/den)                          */
    int64_t G;
    int32_t R;
    int32_t lines;       /* bit 0: the plan also holds the whole-line chunking for fp32 (time, gridcell) data (lines of 32 cells);
                            bit 1: the one for fp64 data (lines of 16 cells); bit 2: the 64-cell one of fp64 degree days (four
                            lines of 16 cells: both fields of a chunk in one image).  All serve the loader/consumer kernel.       */
    int64_t n_lines128;  /* sum over chunks of distinct 128-byte lines (32 fp32 cells) their quads touch */
    int64_t n_sectors64; /* ... of distinct 64-byte sectors */
    /* whole-line chunkings (else 0): chunks of eight whole 128-byte lines (32 fp32 / 16 fp64 cells) of one column strip */
    int64_t n_partial_rows; /* (chunk, region) partial sums = rows of the partial buffer that combine_parts_kernel adds up */
    int64_t lines_chunks;   /* its chunks                                                                               */
    int64_t lines_ucells;   /* cells it fetches per timestep (every line whole, each exactly once)                      */
    int64_t lines_lines128; /* distinct 128-byte lines per timestep (= lines_ucells / 32 on grids of whole lines)       */
    int64_t n_partial_rows64; /* the same three for the fp64 chunking (16-cell lines)                                   */
    int64_t lines64_chunks;
    int64_t lines64_ucells;
} wagg_plan_info;

/* ---- process / device ------------------------------------------------------------------- */
int wagg_version(void);                 /* 10000*major + 100*minor + patch; 0.4.0: sized struct getters, wagg_apply_desc,
                                           wagg_host_stats has 18 fields; 0.5.0: many-plans (wagg_plan_create_many);
                                           0.9.0: packed rows (wagg_pack_rows_*, WAGG_APPLY_COMPACT_ROWS);
                                           0.13.0: spell statistics (wagg_spell_reduce_*);
                                           0.14.0: rolling-window extremes (wagg_rolling_reduce_*);
                                           0.15.0: period quantiles (wagg_quantile_select_*);
                                           0.16.0: spells against per-cell thresholds (wagg_cell_spells_*);
                                           0.17.0: ... with a threshold plane per row (wagg_row_cell_spells_*);
                                           0.18.0: spells that run across period boundaries (wagg_spell_span_*) */
int wagg_device_count(void);            /* number of visible HIP devices (0 if none), never <0  */
/* Time-axis sharding rule of the multi-GPU form (one process per GPU; climate_toolbox_amd/timeshard.py):
 * rank `rank` of `world` owns rows [*start, *stop) of T; the first T mod world ranks hold one row more. */
int wagg_shard_rows(int64_t T, int world, int rank, int64_t *start, int64_t *stop);
const char *wagg_last_error(void);      /* thread-local, never NULL                              */

/* ---- in-library kernel timing (HIP events on the stream the kernel is launched on) ----------- */
/* While enabled, every apply hands an event pair to the launch of its DOMINANT kernel (sparse: the
 * gather kernel; dense-family: the MFMA / entry-list kernel) -- hipExtLaunchKernel's startEvent / stopEvent, which
 * stamp the dispatch itself, so host time between two API calls is never booked as kernel time -- from a
 * ring of WAGG_PROFILE_SLOTS pairs, without any synchronisation.  wagg_profile_read blocks until the recorded
 * kernels have finished and returns their durations in milliseconds, oldest first.  Process-global and not
 * thread-safe: enable/read from the thread that issues the applies.  Not for use under stream capture.   */
#define WAGG_PROFILE_SLOTS 1024
int wagg_profile_enable(int on);        /* also resets the ring */
int wagg_profile_read(float *ms_out, int max_out, int *n_out);
/* The floor of that clock: median (and minimum) of what `n` (1..256) event pairs read for a kernel that does nothing,
 * launched on `stream` the same way.  rocprofv3's dispatch durations (profiles/) do not contain it; sub-millisecond
 * kernels therefore read a few percent longer through wagg_profile_read than there.  Blocks until the launches finished. */
int wagg_profile_event_overhead(void *stream, int n, float *median_ms, float *min_ms /* may be NULL */);

/* ---- label work ahead of the plan (host only) ------------------------------------- */
/* Exact-equality join of the segment table's lat/lon labels to the grid's (Dataset.sel without
 * method=, aggregations.py:27): cell_idx[i] = ilat*nlon + ilon (or ilon*nlat + ilat when lon_major).
 * WAGG_EKEY with *bad_row = first row whose label is absent; grid labels must be unique.          */
int wagg_resolve_cells(const double *lat, int64_t nlat, const double *lon, int64_t nlon,
                       const double *seg_lat, const double *seg_lon, int64_t nseg, int lon_major,
                       int32_t *cell_idx, int64_t *bad_row);
/* w_eff[i] = w[i] > 0 ? w[i] : backup[i]   (aggregations.py:73: NaN, 0 and negative take the row's backup) */
int wagg_backup_fill(const double *w, const double *backup, int64_t n, double *w_eff);
/* values[i] == from -> to   (aggregations.py:144: pix_cent_x 180.125 -> -179.875) */
int wagg_relabel(double *values, int64_t n, double from, double to);
/* sorted unique labels and per-row codes (-1 for null rows), aggregations.py:78 group keys (S3) */
int wagg_factorize_i64(const int64_t *labels, const uint8_t *isnull, int64_t n, int32_t *codes,
                       int64_t *uniq, int64_t *n_uniq);
int wagg_factorize_bytes(const char *buf, int64_t width, const uint8_t *isnull, int64_t n,
                         int32_t *codes, int64_t *uniq_rows, int64_t *n_uniq);

/* ---- sparse plan: replaces aggregations.py:24-27 + :64-71 (gather index, labels, weights) --- */
/* cell_idx[i]    flat grid cell of segment row i  = ilat*nlon + ilon            (0 <= . < G)
 * region_code[i] rank of the row's label among the sorted unique labels, -1 = null label (S3)
 * w_eff[i]       fp64 weight after the per-row backup fill of :73; NaN rows leave both sums
 * row_len        cells per grid row (nlon), 0 = unknown.  Known (and a whole number of 4-cell quads, G a whole number of
 *                rows), compact tables get a second, whole-line chunking next to the region-shaped one: chunks of eight
 *                whole 128-byte lines of one 32-cell column strip, every line fetched exactly once, regions cut by chunk
 *                borders summed from partial rows -- what fp32 (time, gridcell) applies use (their kernel is bound by
 *                line requests); everything else keeps the region-shaped chunks (fewer bytes)
 * flags          0, or WAGG_PLAN_* bits that pin the kernel form for this plan (tests, ablations);
 *                resolved here, once -- the library reads no environment variable
 * Host pointers; copied.  Duplicate (cell, region) rows add (S5).                              */
#define WAGG_PLAN_NO_LC 1     /* (time, gridcell) data: the persistent one-role kernel instead of the loader/consumer kernels */
#define WAGG_PLAN_NO_STREAM 2 /* every group through the chunk-walking kernel */
#define WAGG_PLAN_NO_LINES 4  /* region-shaped chunks only (rounds 1-2) even where the whole-line chunkings apply */
#define WAGG_PLAN_LC_MFMA 8   /* DIAGNOSTIC BUILD ONLY (libwagg_diag.so): fp32 loader/consumer kernel with dense-tile MFMA consumers
                                 (rounds 1-2) -- the one kernel with a bounded-spin barrier; libwagg.so refuses the flag with
                                 WAGG_EUNSUPPORTED */
#define WAGG_PLAN_SERIAL_BUILD 16 /* build the chunkings one after the other on the calling thread (the library starts three
                                 worker threads otherwise and falls back to exactly this when a thread cannot be started);
                                 the plan is the same bit for bit */
int wagg_plan_create(const int32_t *cell_idx, const int32_t *region_code, const double *w_eff,
                     int64_t nseg, int64_t G, int32_t R, int64_t row_len, int flags,
                     wagg_plan **out);
int wagg_plan_destroy(wagg_plan *plan);
int wagg_plan_get_info(const wagg_plan *plan, wagg_plan_info *info);
int wagg_plan_get_den(const wagg_plan *plan, double *den_host /* R values */); /* :79 */
/* Blocks until `stream` is idle, then reports whether any apply on this plan failed on the device.  No kernel of
 * libwagg.so can: none waits on another wave's progress (the diagnostic build's MFMA-consumer kernel can time out at its
 * consumer barrier: WAGG_EHIP, results incomplete -- there the same check also runs at the start of every later apply on the
 * plan and inside the *_host_ forms, so a device-side failure surfaces as a status, never as silent garbage).          */
int wagg_plan_status(const wagg_plan *plan, void *stream);

/* ---- apply: replaces aggregations.py:78-80 (and the gather of :27, fused) ------------------ */
/* out[t, r] = sum_i X[t, cell_i] * w_i / den[r]; NaN products count as 0 (skipna, S6); den == 0
 * gives IEEE NaN/inf (S7).  f32 accumulates in fp32 (declared deviation from S8, 1e-4 rel),
 * f64 in fp64 (1e-6 rel).  T may be any size >= 0.                                             */
int wagg_apply_f32(const wagg_plan *plan, const float *X_dev, int64_t T, int64_t ldx, int layout,
                   float *out_dev, int64_t ldo, int out_layout, void *stream);
int wagg_apply_f64(const wagg_plan *plan, const double *X_dev, int64_t T, int64_t ldx, int layout,
                   double *out_dev, int64_t ldo, int out_layout, void *stream);
/* Blocking forms on host buffers.  (time, gridcell) data with a (time, region) result is
 * streamed through the device in row blocks of ~256 MiB: the H2D copy of block i+1, the kernels of block i
 * and the return of block i-1's result run on three streams at once, and the device holds two blocks at a
 * time (host arrays of c4 / c5 size, 45-76 GB, need no device copy of the whole field).  flags:
 *   WAGG_HOST_PIN    page-lock the caller's arrays in place for the call (hipHostRegister / hipHostUnregister,
 *                    both statuses checked) so that the copy engines read and write them directly
 *   WAGG_HOST_WHOLE  one copy of the whole field, one apply, one copy back (the other layouts always do)
 * A caller array that is page-locked already (hipHostMalloc, the caller's own hipHostRegister, a framework's pinned
 * allocator) is used as it is, whatever its size -- the drop-in hands in result arrays from its pool of such blocks.
 * What is not page-locked -- arrays below 32 MiB (registration locks whole pages, which a small heap array
 * shares with unrelated objects), arrays whose registration the runtime refuses, and everything without
 * WAGG_HOST_PIN -- passes through the library's own page-locked staging pieces by CPU copy.  A pageable caller
 * pointer is never handed to a runtime copy: the runtime would page-lock the range on the fly and keep that
 * pin, keyed by address, beyond the call (docs/HISTORY.md (f)).  Every HIP status on this path is checked; failures
 * while resources are released are counted (wagg_host_stats) and fail the call.
 * Pitched arrays (ldx > G, ldo > R) are honoured: nothing behind the used cells of the last row is read and the
 * padding between result rows is not written.  The plan must live on the current device.
 * wagg_apply_host_* = the _ex form with WAGG_HOST_PIN | WAGG_HOST_LINES.  Measured on one MI355X (tools/host_path_timing.py):
 * the segment-table form is PCIe-bound either way (1.5 GB field: 51 ms whole from pageable memory, 29.8 ms pinned blocks =
 * 51 GB/s of X, 21.3 ms lines only; the 3 GB fp64 field: 59.2 / 33.5 ms);
 * a dense 1,369-row shard takes 602 ms whole and 523 ms in pinned blocks (the copies hide behind the 490 ms of
 * MFMA work).                                                                                         */
#define WAGG_HOST_PIN 1
#define WAGG_HOST_WHOLE 2
/*   WAGG_HOST_LINES  "lines only" (round 5; segment-table plans, (time, gridcell) data, (time, region) result, one device):
 *                    the table references a fraction of the grid -- the whole 128-byte lines its cells lie in are 64 % of a
 *                    c2-real fp32 row, 47 % of a fp64 row -- so up to twelve host threads (all but four of the CPUs the calling
 *                    thread is granted -- affinity mask and cgroup quota --, at least half of them) pack exactly those runs of every row side by side into a ring of
 *                    page-locked pieces, only the packed rows cross PCIe, and the kernel reads them through a second cell
 *                    table of the same plan.  X is read by the CPU and never page-locked; the result returns as WAGG_HOST_PIN
 *                    says.  Taken when the packed row is <= 80 % of the row, the field >= 64 MiB and the calling thread's
 *                    affinity mask and quota leave enough threads to pack faster than PCIe would move the whole rows (6 x the
 *                    packed fraction, e.g. 4 for c2-real fp32: >= 8 usable CPUs); otherwise (and when the ring is busy with
 *                    a concurrent call, or the threads cannot be started) the call runs as without the flag:
 *                    the flag permits, it never fails a call.  Same bits as every other form (the kernel sees the same cells
 *                    in the same order).  wagg_host_stats.lines_h2d_bytes counts the packed bytes sent.
 *                    Measured (tools/host_path_timing.py, c2-real T = 365): fp32 29.8 -> 21.3 ms per call (the C call alone
 *                    18.5 ms, of which 16.7 ms are the copy engine's), fp64 59.2 -> 33.5 ms; docs/HISTORY.md (f).              */
#define WAGG_HOST_LINES 4
/*   WAGG_HOST_LINES_WHOLE  with WAGG_HOST_LINES: pack the whole 128-byte lines as in round 5.  Without it (round 6, "quads
 *                    only") the packed row holds only the 16-byte QUADS that contain a referenced cell -- a whole-line chunk
 *                    fetches every quad of its lines, but the kernel reads only those; the others are pointed at a valid
 *                    dummy position -- whenever at least ten packing threads can be had (the runs are shorter: 116 instead of
 *                    455 bytes on c2-real; twelve threads stay ahead of PCIe, eight do not): 33.5 % of a c2-real fp32 row
 *                    instead of 63.6 %, c2-real T = 365 packing + copy 18.1 -> 10.2 ms (tools/host_granule_gonogo.sh,
 *                    profiles/r06_host_granule.txt).  Same kernel, same cells in the same order, and the kernel's choice between
 *                    its finite-data and general accumulation forms looks at REFERENCED quads only: the same bits as the device
 *                    apply for the plain, power and degree-day forms alike.                                              */
#define WAGG_HOST_LINES_WHOLE 8
int wagg_apply_host_f32(const wagg_plan *plan, const float *X_host, int64_t T, int64_t ldx,
                        int layout, float *out_host, int64_t ldo, int out_layout);
int wagg_apply_host_f64(const wagg_plan *plan, const double *X_host, int64_t T, int64_t ldx,
                        int layout, double *out_host, int64_t ldo, int out_layout);
int wagg_apply_host_ex_f32(const wagg_plan *plan, const float *X_host, int64_t T, int64_t ldx,
                           int layout, float *out_host, int64_t ldo, int out_layout, int flags);
int wagg_apply_host_ex_f64(const wagg_plan *plan, const double *X_host, int64_t T, int64_t ldx,
                           int layout, double *out_host, int64_t ldo, int out_layout, int flags);
/* Multi-device form of the above (SURVEY 8b `n_devices`, 8e "one process driving all devices"): plans[s] is a
 * replica of the same table created while device devices[s] was current.  The row blocks of the host field are
 * dealt round-robin to the n_devices pipelines (block i -> slot i mod n_devices, wagg_host_block_plan gives the
 * block size), each driven by its own host thread over its own PCIe link; every block's result lands directly in
 * the caller's rows, so there is no exchange between devices and no collective.  (time, gridcell) data and
 * (time, region) results only; flags: 0 or WAGG_HOST_PIN.  The same device may be listed more than once.       */
int wagg_apply_host_multi_f32(const wagg_plan *const *plans, const int *devices, int n_devices, const float *X_host,
                              int64_t T, int64_t ldx, float *out_host, int64_t ldo, int flags);
int wagg_apply_host_multi_f64(const wagg_plan *const *plans, const int *devices, int n_devices, const double *X_host,
                              int64_t T, int64_t ldx, double *out_host, int64_t ldo, int flags);
/* rows per block and number of blocks of a host field of T rows of row_bytes (= ldx * element size) bytes when a launch
 * handles `quantum` rows well (64: segment-table kernels; 368 / 176: fp32 / fp64 MFMA forms; 128 / 64: entry lists) */
int wagg_host_block_plan(int64_t T, int64_t row_bytes, int64_t quantum, int n_devices, int64_t *block_rows, int64_t *n_blocks);
/* what the host paths did since the last reset (process-wide counters): page-locks taken / refused / released /
 * whose release failed, HIP failures met while releasing resources, bytes moved through the staging pieces and
 * directly from / to page-locked caller memory                                                                      */
typedef struct wagg_host_stats {
    int64_t calls, blocks, registered, register_failed, unregistered, unregister_failed, cleanup_failed;
    int64_t staged_h2d_bytes, staged_d2h_bytes, direct_h2d_bytes, direct_d2h_bytes;
    int64_t lines_h2d_bytes;      /* packed rows of the lines-only path (WAGG_HOST_LINES) ...                              */
    int64_t lines_wait_pack_us;   /* ... time its pipeline thread waited for the packing threads (they are the bottleneck) */
    int64_t lines_wait_copy_us;   /* ... and for the copy engine to hand a ring piece back (PCIe is the bottleneck)        */
    int64_t blocks_retired;       /* calls that ran < 60 % of the best rate (bytes over PCIe / wall time) seen for calls of their
                                     shape: their own device blocks went back to the driver instead of the pool               */
    int64_t found_page_locked;    /* caller arrays that were page-locked already (used as they are, no registration)          */
    int64_t watched_calls;        /* calls the copy-rate watch judged (>= 256 MiB moved from page-locked memory)               */
    int64_t last_rate_permille;   /* the LAST call's copy rate over the best seen for its shape, x 1000 (1000 = it set or met the
                                     record; below 600 the call retired its blocks); 0 = the last call was not judged.  A state,
                                     not a counter: `reset` leaves it                                                          */
} wagg_host_stats;
int wagg_host_stats_read(wagg_host_stats *out, int reset);     /* = the _sized form with sizeof(wagg_host_stats) of THIS header */

/* ---- structs that cross the boundary by layout --------------------------------------------------------------------- */
/* wagg_plan_info, wagg_dense_info, wagg_host_stats and wagg_apply_desc only ever GROW AT THE END.  A binding that mirrors
 * them by hand (ctypes, cffi, cgo) asks the library for its sizes and hands its OWN size to the *_sized getters: the library
 * fills min(size, its own size) bytes and zeroes what the caller has beyond that, so a binding built against an older or a
 * newer header is memory-safe without a version check (fields it does not know are not written; fields the library does
 * not know read 0).  wagg_struct_ordinals writes, into every scalar field in declaration order, its 1-based ordinal (array
 * elements count one each): a binding's self-test that its field ORDER and TYPES are the library's
 * (tests/test_abi.py does exactly that for climate_toolbox_amd/_lib.py).                                                 */
#define WAGG_STRUCT_PLAN_INFO 0
#define WAGG_STRUCT_DENSE_INFO 1
#define WAGG_STRUCT_HOST_STATS 2
#define WAGG_STRUCT_APPLY_DESC 3
int wagg_struct_size(int which);                                   /* sizeof in this library; WAGG_EINVAL for an unknown id */
int wagg_struct_ordinals(int which, void *out, uint64_t size);     /* fills min(size, sizeof) bytes as described above      */
int wagg_plan_get_info_sized(const wagg_plan *plan, void *info, uint64_t size);
int wagg_host_stats_read_sized(void *out, uint64_t size, int reset);

/* ---- fused grid-level transform ---------------------------------------------- */
/* Replaces  tas_poly  (climate_toolbox/transformations/transformations.py:160-208, the arithmetic
 * at :188  ``(ds.tas - 273.15) ** power``) followed by the aggregation above, for the powers
 * p = pow_first .. pow_first + n_pow - 1 in ONE call:
 *   out_p[t, r] = sum_i (X[t, cell_i] + offset)^p * w_eff[i] / den[r].
 * The transform is evaluated in the data type while X is loaded (NaN stays NaN and is skipped
 * like any NaN product, S6), so the transformed grids are never written to memory;
 * (time, gridcell) data, fp32 and fp64, is read from HBM once per four consecutive powers.  The i-th
 * power is stored at out_dev + i * out_pstride (elements) with leading dimension ldo.  Powers must
 * lie in [1, 16]. */
int wagg_apply_poly_f32(const wagg_plan *plan, const float *X_dev, int64_t T, int64_t ldx, int layout,
                        double offset, int pow_first, int n_pow, float *out_dev, int64_t ldo,
                        int64_t out_pstride, int out_layout, void *stream);
int wagg_apply_poly_f64(const wagg_plan *plan, const double *X_dev, int64_t T, int64_t ldx, int layout,
                        double offset, int pow_first, int n_pow, double *out_dev, int64_t ldo,
                        int64_t out_pstride, int out_layout, void *stream);
/* The same for a HOST-resident (time, gridcell) field, (time, region) results in host memory (round 5): the field goes
 * through the row-block pipeline of wagg_apply_host_ex_* once -- every block is raised to its powers on the device, four
 * per pass -- and plane i of the result (power pow_first + i) lands at out_host + i * out_pstride (elements, >= T * ldo)
 * with leading dimension ldo.  flags: WAGG_HOST_PIN, WAGG_HOST_LINES (as there; WAGG_HOST_LINES sends only the 128-byte
 * lines the table references).  This is the reference's tas_poly-then-aggregate on the arrays its callers hold
 * (transformations.py:188 + aggregations.py:87): c2-real, four powers, 1.5 GB field: docs/HISTORY.md (f).  Blocking. */
int wagg_apply_poly_host_f32(const wagg_plan *plan, const float *X_host, int64_t T, int64_t ldx, double offset, int pow_first,
                             int n_pow, float *out_host, int64_t ldo, int64_t out_pstride, int flags);
int wagg_apply_poly_host_f64(const wagg_plan *plan, const double *X_host, int64_t T, int64_t ldx, double offset, int pow_first,
                             int n_pow, double *out_host, int64_t ldo, int64_t out_pstride, int flags);

/* Replaces  snyder_edd  (transformations.py:7-93: Snyder exceedance degree days of the daily
 * (tasmin, tasmax) pair at a threshold e, the nested xr.where of :75-87) followed by the
 * aggregation, for n_thr thresholds in one call.  Both fields have the layout/ldx of X above and
 * are shifted by `offset` first (-273.15 for Kelvin files; the thresholds are in the shifted
 * unit).  Threshold i is stored at out_dev + i * out_pstride.  snyder_gdd (:96-144) is the
 * difference of two of these outputs (the aggregation is linear).                               */
int wagg_apply_edd_f32(const wagg_plan *plan, const float *tasmin_dev, const float *tasmax_dev, int64_t T,
                       int64_t ldx, int layout, double offset, const double *thresholds, int n_thr,
                       float *out_dev, int64_t ldo, int64_t out_pstride, int out_layout, void *stream);
int wagg_apply_edd_f64(const wagg_plan *plan, const double *tasmin_dev, const double *tasmax_dev, int64_t T,
                       int64_t ldx, int layout, double offset, const double *thresholds, int n_thr,
                       double *out_dev, int64_t ldo, int64_t out_pstride, int out_layout, void *stream);
/* The same for two HOST-resident (time, gridcell) fields, (time, region) results in host memory (round 5): tasmin and tasmax go
 * through the row-block pipeline of wagg_apply_host_ex_* together, every block's degree days are evaluated on the device (four
 * thresholds per pass over the block) and plane i (threshold i) lands at out_host + i * out_pstride (elements, >= T * ldo).
 * flags: WAGG_HOST_PIN, WAGG_HOST_LINES (only the lines of both fields the table references cross PCIe).  Blocking.  This is
 * snyder_edd-then-aggregate (transformations.py:7-93 + aggregations.py:87) on the arrays the reference's callers hold.      */
int wagg_apply_edd_host_f32(const wagg_plan *plan, const float *tasmin_host, const float *tasmax_host, int64_t T, int64_t ldx,
                            double offset, const double *thresholds, int n_thr, float *out_host, int64_t ldo,
                            int64_t out_pstride, int flags);
int wagg_apply_edd_host_f64(const wagg_plan *plan, const double *tasmin_host, const double *tasmax_host, int64_t T, int64_t ldx,
                            double offset, const double *thresholds, int n_thr, double *out_host, int64_t ldo,
                            int64_t out_pstride, int flags);

/* ---- materialised grid-level transforms (device buffers, elementwise) ------------------------ */
/* What ``.values`` of a lazily transformed variable returns: out[i] = (X[i] + offset)^power
 * (transformations.py:188), out[i] = sum_k coefs[k] * snyder_edd(tasmin[i] + offset, tasmax[i] + offset,
 * thresholds[k]) (transformations.py:64-87; two terms with coefs +1/-1 = snyder_gdd, :138-140), with the
 * device functions the fused aggregation kernels use.  n_terms <= 8.  wagg_any_less_* is the check of
 * transformations.py:62 (``assert not (tasmax < tasmin).any()``): *result = 1 iff some a[i] < b[i]; blocks. */
int wagg_transform_poly_f32(const float *X_dev, int64_t n, double offset, int power, float *out_dev, void *stream);
int wagg_transform_poly_f64(const double *X_dev, int64_t n, double offset, int power, double *out_dev, void *stream);
int wagg_transform_edd_f32(const float *tasmin_dev, const float *tasmax_dev, int64_t n, double offset,
                           const double *coefs, const double *thresholds, int n_terms, float *out_dev, void *stream);
int wagg_transform_edd_f64(const double *tasmin_dev, const double *tasmax_dev, int64_t n, double offset,
                           const double *coefs, const double *thresholds, int n_terms, double *out_dev, void *stream);
/* out[i] = sum_k coefs[k] * planes[k * plane_stride + i], n_planes <= 8: several aggregated planes combined into one
 * (snyder_gdd = EDD(threshold_low) - EDD(threshold_high), transformations.py:138-140, after the aggregation: it is linear) */
int wagg_combine_planes_f32(const float *planes_dev, int n_planes, int64_t plane_stride, const double *coefs, int64_t n,
                            float *out_dev, void *stream);
int wagg_combine_planes_f64(const double *planes_dev, int n_planes, int64_t plane_stride, const double *coefs, int64_t n,
                            double *out_dev, void *stream);
/* Data movement of device-resident fields in front of the path.  wagg_take_axis: dst[o][i][:] = src[o][idx[i]][:] for a
 * contiguous array seen as (outer, n_src, inner_bytes) -- the 29-February drop along time (utils.py:60-74) and the lon
 * re-ordering (utils.py:33-40); idx_dev is an int64 device array, inner_bytes a multiple of 4.  wagg_relayout_*: dst
 * (contiguous, shape[0..ndim)) <- src with element strides src_strides (any permutation of up to 6 dims: the transpose of a
 * field whose lat/lon axes are not adjacent).                                                                            */
int wagg_take_axis(const void *src_dev, int64_t outer, int64_t n_src, int64_t inner_bytes, const int64_t *idx_dev,
                   int64_t n_idx, void *dst_dev, void *stream);
int wagg_relayout_f32(const float *src_dev, int ndim, const int64_t *shape, const int64_t *src_strides, float *dst_dev, void *stream);
int wagg_relayout_f64(const double *src_dev, int ndim, const int64_t *shape, const int64_t *src_strides, double *dst_dev, void *stream);
/* a device field of another element type as a contiguous fp64 array (the reference's own promotion: any dtype times float64
 * weights is float64, S8), strided source as for wagg_relayout_* with strides in elements of the source type */
#define WAGG_T_F16 0
#define WAGG_T_BF16 1
#define WAGG_T_I8 2
#define WAGG_T_U8 3
#define WAGG_T_I16 4
#define WAGG_T_I32 5
#define WAGG_T_I64 6
#define WAGG_T_F32 7
#define WAGG_T_F64 8
int wagg_relayout_to_f64(const void *src_dev, int src_type, int ndim, const int64_t *shape, const int64_t *src_strides,
                         double *dst_dev, void *stream);
/* One blocking copy of a contiguous host buffer to the device, the way the library uploads its own operands: buffers of
 * >= 32 MiB are page-locked in place for the copy (one DMA; the lock goes before the call returns), smaller ones pass through
 * the library's page-locked staging pieces -- a pageable pointer is never handed to a runtime copy, which pins the range on
 * the fly and keeps that pin, keyed by address, beyond the call.  Measured (tools/host_edd_timing.py, 1.5 GB): 32.4 ms =
 * 47 GB/s lock + copy + unlock, the same as a runtime copy of an array the runtime has pinned in an earlier call (32.8 ms;
 * its first copy of a new array is slower).  The drop-in uploads the host-resident fields the row-block pipelines do not
 * serve (degree days, (gridcell, time) data, dense-family plans with transforms) through it.                                */
int wagg_upload(void *dst_dev, const void *src_host, int64_t bytes);
int wagg_any_less_f32(const float *a_dev, const float *b_dev, int64_t n, int *result, void *stream);
int wagg_any_less_f64(const double *a_dev, const double *b_dev, int64_t n, int *result, void *stream);

/* ---- materialised gather: what _reindex_spatial_data_to_regions returns (:27) -------------- */
/* out[t, i] = X[t, cell_idx[i]] in out_layout (WAGG_OUT_TR: out[t*ldo+i], RT: out[i*ldo+t]).   */
int wagg_gather_f32(const float *X_dev, int64_t T, int64_t ldx, int layout,
                    const int32_t *cell_idx_dev, int64_t nseg, float *out_dev, int64_t ldo,
                    int out_layout, void *stream);
int wagg_gather_f64(const double *X_dev, int64_t T, int64_t ldx, int layout,
                    const int32_t *cell_idx_dev, int64_t nseg, double *out_dev, int64_t ldo,
                    int out_layout, void *stream);

/* ---- dense weights: W[g, r] as an fp32 matrix resident in HBM, MFMA contraction ------------- */
/* synth: W[g,r] = hash_u01(g*R + r, seed) in [0,1), generated on device (never on host); this is
 * the c2-dense benchmark operand (1,036,800 x 24,378 = 101 GB).                                */
int wagg_dense_create_synth(int64_t G, int32_t R, uint32_t seed, wagg_dense **out);
/* the same with only a fraction `fill` of the entries non-zero, at uniformly random positions
 * (kept where hash_u01(g*R + r, seed ^ 0x9e3779b9) < fill): c5's "uniform-random columns"
 * structure at fill = 0.01 -- no tile of W is empty, yet 99 % of every tile is.                 */
int wagg_dense_create_synth_sparse(int64_t G, int32_t R, uint32_t seed, double fill, wagg_dense **out);
/* (fill < 10 %: built directly as entry lists, WAGG_FORM_ENTRIES -- c5 at fill = 0.01; above that the
 * full matrix is generated; the same holds for wagg_dense_create_synth_f64)                        */
/* from a host row-major (G, R) fp32 matrix (small cases / tests) */
int wagg_dense_create_host(const float *W_host, int64_t G, int32_t R, wagg_dense **out);
/* from a sparse plan's coded table (weights whose regions are scattered over the grid).  The caller brings ONE kind of
 * table, like the reference (aggregations.py:64-73); which of the three device forms it takes is the library's choice,
 * made from the structure it finds (a census of the occupied (32-cell x 256-region) tiles and the number of distinct
 * pairs) by the estimated time per row of X of each form at its measured rate (tools/form_crossover.py, docs/HISTORY.md (b)):
 * only the non-empty tiles on the MFMA kernel (WAGG_FORM_TILES: c5's block-local weights), entry lists on the vector ALU
 * (WAGG_FORM_ENTRIES: c5's uniformly random 1 %), or the full matrix (WAGG_FORM_FULL).
 * flags: WAGG_DENSE_FORM_AUTO (0), or WAGG_DENSE_FORCE_* to pin the form -- for measurements and tests; results agree
 * between the forms to rounding.  Up to 2^31 - 1 rows.                                              */
#define WAGG_DENSE_FORM_AUTO 0
#define WAGG_DENSE_FORCE_FULL 1
#define WAGG_DENSE_FORCE_TILES 2
#define WAGG_DENSE_FORCE_ENTRIES 3
/* ... or-ed with WAGG_DENSE_GENERAL_SORT: sort the table with the general radix sort even when it is a CSR table with
 * ascending columns, which the builder otherwise puts in order with one stable pass per chunk of 128 cells (the plans
 * are bit-identical; for tests and timings) */
#define WAGG_DENSE_GENERAL_SORT 16
int wagg_dense_create_from_segments(const int32_t *cell_idx, const int32_t *region_code,
                                    const double *w_eff, int64_t nseg, int64_t G, int32_t R,
                                    int flags, wagg_dense **out);
/* The same table in CSR form -- BASELINE configs[4] "sparse CSR weights (<= 1 % nnz)": rows = grid cells (rowptr[G + 1],
 * rowptr[0] = 0, non-decreasing), col = region codes (-1 = null label, dropped), val = fp64 weights (NaN: dropped);
 * columns of a row in any order, repeated (cell, region) pairs add in the order they are stored (S5).
 * Both constructors only UPLOAD the host arrays (page-locked in place for the copy when they are large, through the
 * library's staging pieces otherwise: no host copy of the table is made); sorting into the kernels' order, coalescing,
 * the denominators (aggregations.py:79), the tile census that picks the form, and the packing run on the device
 * (stable radix sort, fixed summation orders: the same table gives the same plan, bit for bit; csrc/wagg_build.hip) --
 * on a stream of the build's own, out of one scratch arena: a build never waits for, nor stops, the streams other plans
 * are applied on.  Up to 2^31 - 1 entries; a configs[4]-sized table (2.53e8 entries, 3 GB) needs ~12 GB of device scratch
 * while it is built (48 bytes per entry) plus 16 bytes per distinct pair.  wagg_dense_info.build_s / build_upload_s
 * report where the time went.                                                                                         */
int wagg_dense_create_from_csr(const int64_t *rowptr, const int32_t *col, const double *val, int64_t G, int32_t R,
                               int flags, wagg_dense **out);
/* synthetic block-local weights (SURVEY 8d, c5 "each 64-cell run touches <= 256 regions"): run j of
 * 64 cells touches the 256 regions of column tile (97 j) mod ceil(R/256); inside, W[g,r] =
 * hash_u01(g*R + r, seed) where hash_u01(g*R + r, seed ^ 0x9e3779b9) < fill, else 0.  Generated on
 * the device in tile-sparse form (benchmark operand; the oracle regenerates it from the hashes).  */
int wagg_dense_create_synth_blocklocal(int64_t G, int32_t R, uint32_t seed, double fill, wagg_dense **out);
#define WAGG_FORM_FULL 0     /* every (32-cell x 256-region) tile of W stored, fp32 MFMA contraction            */
#define WAGG_FORM_TILES 1    /* only the non-empty tiles ("tile-sparse": block-local weights), same MFMA kernel */
#define WAGG_FORM_ENTRIES 2  /* no matrix: per-wave (cell, region, weight) lists, vector-ALU kernel (scattered,
                                sparse weights: a few per cent of non-zeros spread over (almost) every tile), fp32 or fp64 */
/* The *_f64 constructors build the same forms with fp64 weights for fp64 data (the reference's own
 * arithmetic type, aggregations.py:73-80): tiles are (16-cell x 256-region), the contraction runs on
 * v_mfma_f64_16x16x4_f64 (wagg_dense_apply_f64); the entry-list form keeps 64-bit weights (80 bytes per
 * 8 entries instead of 48) and accumulates with v_fma_f64, one timestep per lane.  A plan serves one
 * element type.                                                                                      */
int wagg_dense_create_synth_f64(int64_t G, int32_t R, uint32_t seed, double fill, wagg_dense **out);
int wagg_dense_create_host_f64(const double *W_host, int64_t G, int32_t R, wagg_dense **out);
int wagg_dense_create_from_segments_f64(const int32_t *cell_idx, const int32_t *region_code,
                                        const double *w_eff, int64_t nseg, int64_t G, int32_t R,
                                        int flags, wagg_dense **out);
int wagg_dense_create_from_csr_f64(const int64_t *rowptr, const int32_t *col, const double *val, int64_t G, int32_t R,
                                   int flags, wagg_dense **out);
int wagg_dense_create_synth_blocklocal_f64(int64_t G, int32_t R, uint32_t seed, double fill, wagg_dense **out);
typedef struct wagg_dense_info {
    int64_t G, n_tiles, w_bytes;   /* stored (32 x 256) tiles; bytes of W (or of the entry lists) in HBM */
    int32_t R, n_kt, n_nt, tiled;  /* k tiles, column tiles, 1 = tile-sparse form */
    int32_t form, elem_bytes;      /* WAGG_FORM_*; 4 = fp32 plan, 8 = fp64 plan */
    int64_t nnz;                   /* kept distinct (cell, region) pairs: entry-list form and every plan built from a
                                      caller's table (from_segments / from_csr); else -1 */
    double build_s, build_upload_s; /* plans built from a caller's table: wall seconds of the constructor, and the part of
                                      them spent moving the table to the device (else 0) */
    double est_row_s[3];           /* plans built from a caller's table: what the form choice went by -- estimated seconds per
                                      row of X in the forms WAGG_FORM_FULL / _TILES / _ENTRIES (else 0) */
    int64_t walked_entries;        /* ... and the entries the entry-list kernel would walk (16 x the longest per-wave list of
                                      every (region block, chunk) item): = nnz for evenly spread weights */
    int32_t one_pass_sort, reserved0; /* 1 = the table was put in key order by the one-pass chunk partition (CSR, ascending
                                      columns, nothing dropped), 0 = by the general radix sort */
    int64_t w_image_bytes;         /* full-form fp32 plans: bytes of the f16 high / low image of W that the split apply reads
                                      (= w_bytes, held while the device had room for it at plan time; a clone decides anew on
                                      its own device); 0 = no image: the apply splits W in registers -- same results, bit for
                                      bit.  Applies of more than one row block (T > 368) split in registers either way */
} wagg_dense_info;
int wagg_dense_get_info(const wagg_dense *d, wagg_dense_info *info);
int wagg_dense_get_info_sized(const wagg_dense *d, void *info, uint64_t size);   /* see "structs that cross the boundary by layout" */
/* Device blocks and streams the library needs for the length of one call -- the arena of a table -> plan build (11 GB for
 * a 2.5e8-row table), the block buffers and streams of a host-resident apply, a plan's per-stream staging -- come from a
 * per-device pool and return to it (csrc/wagg_scratch.hip: giving 11 GB back to the driver and asking again costs a wait
 * of seconds every dozen builds).  At most 1/16 of a device's memory is kept.  This frees it (the package's
 * clear_caches() calls it); an allocation of the library that runs out of device memory does so by itself before it
 * tries once more. */
int wagg_release_scratch(void);
int64_t wagg_scratch_bytes(void);  /* device bytes kept right now, all devices */
/* A second plan with the same weights on `device` (may be the device `src` lives on): the finished plan's device arrays --
 * packed W with its tile tables, or the entry lists, and the denominators -- are copied device to device (hipMemcpyPeer:
 * xGMI between two GPUs), nothing is uploaded or sorted again and no host copy of the caller's table is needed.  The
 * clone owns its workspaces, so the two plans apply independently (wagg_apply_host_multi_* wants one plan per pipeline).
 * `src` is only read: applies on it may be in flight.  The calling thread's current device is left as it was. */
int wagg_dense_clone(const wagg_dense *src, int device, wagg_dense **out);
int wagg_dense_destroy(wagg_dense *d);
int wagg_dense_get_den(const wagg_dense *d, double *den_host /* R values */);
/* Diagnostic entry (layout tests; a library built from an older header lacks it): the stored tiles as they lie on the device, to
 * a host buffer of exactly w_bytes -- image = 0 the packed W, 1 the f16 high / low image of a full-form fp32 plan (WAGG_EINVAL
 * when the plan holds none).  image = 2 / 3: the first `bytes` of the split form's workspaces as the last apply of the plan
 * left them (the caller has waited for it): 2 the packed f16 high / low tiles of X, 3 the row maxima as float bits, one a
 * row.  Not for entry-list plans. */
int wagg_dense_read_w(const wagg_dense *d, int image, void *host, uint64_t bytes);
/* out[t, r] = sum_g nan0(X[t,g]) * W[g,r] / den[r], fp32 MFMA (v_mfma_f32_16x16x4_f32).
 * ksplit = 0 picks the k-slice count; otherwise a multiple of 8.  The plan owns the packed copy of
 * X and the partial-sum slabs of an apply (hence the non-const handle): applies on ONE dense plan
 * must be ordered on one stream; different plans are independent.
 * Tile-sparse plans (and full ones with two or more tall row blocks) read X where it lies when its rows
 * are 16-byte aligned and G is a whole number of k tiles (32 floats / 16 doubles): no packed copy is written; a field with NaN
 * or +-inf in it is noticed on the device (non-finite numerators) and redone through the packed
 * pass on the same stream, so the result and wagg_dense_saw_inf are the same either way; after that
 * the plan keeps to the packed pass.                                                              */
int wagg_dense_apply_f32(wagg_dense *d, const float *X_dev, int64_t T, int64_t ldx,
                         float *out_dev, int64_t ldo, int ksplit, void *stream);
/* fp64 data on an fp64 plan: out = sum_g nan0(X[t,g]) * W[g,r] / den[r] on v_mfma_f64_16x16x4_f64 */
int wagg_dense_apply_f64(wagg_dense *d, const double *X_dev, int64_t T, int64_t ldx,
                         double *out_dev, int64_t ldo, int ksplit, void *stream);
/* the same contraction of (X + offset)^power (tas_poly, transformations.py:188) and of
 * snyder_edd(tasmin + offset, tasmax + offset, threshold) (transformations.py:64-87): the transform is
 * evaluated while X is packed, the transformed grid is never written anywhere                    */
int wagg_dense_apply_poly_f32(wagg_dense *d, const float *X_dev, int64_t T, int64_t ldx, double offset,
                              int power, float *out_dev, int64_t ldo, int ksplit, void *stream);
int wagg_dense_apply_edd_f32(wagg_dense *d, const float *tasmin_dev, const float *tasmax_dev, int64_t T,
                             int64_t ldx, double offset, double threshold, float *out_dev, int64_t ldo,
                             int ksplit, void *stream);
int wagg_dense_apply_poly_f64(wagg_dense *d, const double *X_dev, int64_t T, int64_t ldx, double offset,
                              int power, double *out_dev, int64_t ldo, int ksplit, void *stream);
int wagg_dense_apply_edd_f64(wagg_dense *d, const double *tasmin_dev, const double *tasmax_dev, int64_t T,
                             int64_t ldx, double offset, double threshold, double *out_dev, int64_t ldo,
                             int ksplit, void *stream);
/* host-resident (time, gridcell) data through a dense-family plan, row-block pipeline as wagg_apply_host_ex_* */
int wagg_dense_apply_host_f32(wagg_dense *d, const float *X_host, int64_t T, int64_t ldx,
                              float *out_host, int64_t ldo, int flags);
int wagg_dense_apply_host_f64(wagg_dense *d, const double *X_host, int64_t T, int64_t ldx,
                              double *out_host, int64_t ldo, int flags);
/* ... and over several devices, one replica of the plan per device (as wagg_apply_host_multi_*; a dense-family plan
 * owns its workspaces, so every slot needs a replica of its own).  The +-inf notes of all replicas (wagg_dense_saw_inf)
 * are collected in plans[0] before the call returns and cleared in the others.                                       */
int wagg_dense_apply_host_multi_f32(wagg_dense *const *plans, const int *devices, int n_devices, const float *X_host,
                                    int64_t T, int64_t ldx, float *out_host, int64_t ldo, int flags);
int wagg_dense_apply_host_multi_f64(wagg_dense *const *plans, const int *devices, int n_devices, const double *X_host,
                                    int64_t T, int64_t ldx, double *out_host, int64_t ldo, int flags);
/* The MFMA forms multiply every (cell, region) pair of a stored tile, so +-inf in the (transformed)
 * data turns the zero weights of regions that do not own the cell into NaN, where the reference and
 * the segment-table form confine it to the owning regions (S6).  The pack stage notes such data:
 * this call synchronises `stream`, returns in *saw whether any apply since the last call met +-inf
 * and clears the note; the caller then repeats that field through a wagg_plan.  (The entry-list
 * form multiplies real pairs only and never sets it.)                                            */
int wagg_dense_saw_inf(wagg_dense *d, void *stream, int *saw);

/* ---- synthetic data generators (device side, shared with the CPU oracle bit for bit) ------- */
/* The c5 weight tables of wagg_dense_create_synth_sparse (blocklocal = 0) / _synth_blocklocal (1) as a caller would hand
 * them in: CSR on the HOST (rows = cells, columns ascending, fp64 values = the fp32 hashes).  Generated on the device and
 * copied out; call with col_host = val_host = NULL first to get rowptr and *nnz_out, then with arrays of that capacity.  */
int wagg_synth_table_csr(int64_t G, int32_t R, uint32_t seed, double fill, int blocklocal, int64_t *rowptr_host,
                         int32_t *col_host, double *val_host, int64_t capacity, int64_t *nnz_out);
/* X[t*ldx + g] = base + amp * (hash_u01(t*G + g, seed) - 0.5)                                   */
int wagg_synth_field_f32(float *X_dev, int64_t T, int64_t G, int64_t ldx, uint32_t seed,
                         float base, float amp, void *stream);
int wagg_synth_field_f64(double *X_dev, int64_t T, int64_t G, int64_t ldx, uint32_t seed,
                         double base, double amp, void *stream);

/* ---- time-axis shards on several devices, ONE process, device-resident data (SURVEY 8b n_devices, 8e) ----------------
 * Output row t depends on input row t only: shard i (rows_i rows of the job, resident on devices[i]) goes through plans[i]
 * on devices[i]; its (rows_i x R) block lands directly in rows [sum_{j<i} rows_j, ...) of out_root on devices[root].  No
 * exchange during compute; one at the end, by `transport`:
 *   WAGG_GATHER_RCCL  grouped ncclSend / ncclRecv between the communicators of ncclCommInitAll: every shard -> root on its
 *                     own xGMI link (a direct gather, not a ring).  librccl is looked up at run time, not linked: the copy
 *                     the process already holds (torch's) if there is one.  Every device once; out_root rows contiguous.
 *   WAGG_GATHER_PEER  peer copies (hipMemcpyPeerAsync / hipMemcpy2DAsync) on the shard's own stream: needs no library, takes
 *                     pitched results, and allows a device to be listed twice (several shards on one GPU)
 *   WAGG_GATHER_AUTO  RCCL when it can be loaded, the devices are distinct and n > 1; else peer copies
 * A group owns one stream per shard and the shards' staging blocks; the apply calls are BLOCKING (the result is complete on
 * return) and restore the caller's current device.  The plans are replicas of one table, one per shard (a dense-family plan
 * owns its workspaces; a segment-table plan may serve several shards of its own device).  The process-per-GPU form of the
 * same job is torch.distributed + RCCL (climate_toolbox_amd/timeshard.py); for host-resident fields see
 * wagg_*_apply_host_multi_*.  Validated on hardware with several shards on ONE device (peer copies) and with RCCL at n = 1;
 * unmeasured at n > 1 devices (gpurun exposes one GPU).                                                                  */
typedef struct wagg_shard_group wagg_shard_group;
#define WAGG_GATHER_AUTO 0
#define WAGG_GATHER_RCCL 1
#define WAGG_GATHER_PEER 2
int wagg_shard_group_create(const int *devices, int n, int transport, wagg_shard_group **out);
int wagg_shard_group_destroy(wagg_shard_group *g);
int wagg_shard_group_info(const wagg_shard_group *g, int *n_shards, int *transport /* RCCL or PEER: what the group uses */);
int wagg_apply_sharded_f32(wagg_shard_group *g, const wagg_plan *const *plans, const float *const *X_dev, const int64_t *rows,
                           int64_t ldx, float *out_root, int64_t ldo, int root);
int wagg_apply_sharded_f64(wagg_shard_group *g, const wagg_plan *const *plans, const double *const *X_dev, const int64_t *rows,
                           int64_t ldx, double *out_root, int64_t ldo, int root);
int wagg_dense_apply_sharded_f32(wagg_shard_group *g, wagg_dense *const *plans, const float *const *X_dev, const int64_t *rows,
                                 int64_t ldx, float *out_root, int64_t ldo, int root);
int wagg_dense_apply_sharded_f64(wagg_shard_group *g, wagg_dense *const *plans, const double *const *X_dev, const int64_t *rows,
                                 int64_t ldx, double *out_root, int64_t ldo, int root);

/* ---- one entry point for every apply (round 6) ------------------------------------------------------------------- */
/* Every wagg_*apply* function above is a three-line wrapper that fills this descriptor and calls wagg_apply(): a new
 * transform or a new kind of source is a new VALUE of a field here, not eight new symbols.  New bindings should call
 * wagg_apply() only (INTEGRATION.md section 2 shows both forms; climate_toolbox_amd/engine.py uses nothing else).
 *
 *   struct_size  sizeof(wagg_apply_desc) of the header the caller was built against (the struct only grows at the end;
 *                fields beyond the caller's size read 0 = "not given")
 *   plan_kind    WAGG_PLAN_SEGMENT: `plan` is a wagg_plan*;  WAGG_PLAN_DENSE: a wagg_dense*
 *   elem         WAGG_T_F32 / WAGG_T_F64: element type of x, x2 and out (a dense-family plan must have been built for it)
 *   source       where the field lies and who moves it:
 *                  WAGG_SRC_DEVICE      device pointers, asynchronous on `stream`             (wagg_apply_f32 ...)
 *                  WAGG_SRC_HOST        host arrays through the row-block pipeline, blocking; `flags` = WAGG_HOST_*
 *                  WAGG_SRC_HOST_MULTI  the same over `n_plans` plan replicas on `devices[]`; `plan` is an ARRAY of handles
 *                  WAGG_SRC_SHARDED     `plan` = array of n_plans handles, `x` = array of n_plans device pointers (shard i on
 *                                       the device of plan i), rows[i] rows each; results gathered into `out` on shard `root`
 *                                       of `group` (a wagg_shard_group*); blocking
 *   transform    WAGG_XF_NONE; WAGG_XF_POLY: (x + offset)^p for p = pow_first .. pow_first + n_pow - 1, plane i at
 *                out + i * out_pstride; WAGG_XF_EDD: Snyder degree days of (x = tasmin, x2 = tasmax) + offset at
 *                thresholds[0 .. n_thr), plane i at out + i * out_pstride.  (Dense-family plans: one power / one threshold
 *                per call.)
 *   T, ldx, layout / out, ldo, out_layout   as in wagg_apply_f32 (dense-family plans: WAGG_LAYOUT_TG / WAGG_OUT_TR only)
 *   ksplit       dense-family plans: k-slice count, 0 = the library's choice
 *   flags        WAGG_HOST_* for the host sources; with a dense-family plan also WAGG_APPLY_EXACT_F32 (sources DEVICE and
 *                HOST): an fp32 full-form plan then runs the fp32 MFMA kernel, bit for bit what library 0.5.0 computed,
 *                instead of the default split form (f16 high + low parts of both operands, power-of-two scaled, fp32
 *                accumulation: DESIGN.md gives the error bound).  No effect on other forms or on fp64 plans.
 *                WAGG_APPLY_COMPACT_ROWS (0.9.0): x holds PACKED rows (wagg_pack_rows_*: ldx >= Gq, field 0 of a row) instead of
 *                grid rows.  A single segment-table plan that has the compact row for `elem`, WAGG_SRC_DEVICE, WAGG_LAYOUT_TG in,
 *                WAGG_OUT_TR out, WAGG_XF_NONE only: the kernel of the lines-only host path reads the rows through the plan's
 *                quads-only cell table -- the same cells in the same order as a plain apply of the unpacked rows, the same bits.
 *                With anything else the bit is WAGG_EUNSUPPORTED.
 * A combination the library has no kernel path for returns WAGG_EUNSUPPORTED with a message that names it; nothing is
 * emulated.                                                                                                            */
#define WAGG_PLAN_SEGMENT 0
#define WAGG_PLAN_DENSE 1
#define WAGG_SRC_DEVICE 0
#define WAGG_SRC_HOST 1
#define WAGG_SRC_HOST_MULTI 2
#define WAGG_SRC_SHARDED 3
#define WAGG_XF_NONE 0
#define WAGG_XF_POLY 1
#define WAGG_XF_EDD 2
#define WAGG_APPLY_EXACT_F32 0x10000
#define WAGG_APPLY_COMPACT_ROWS 0x20000
typedef struct wagg_apply_desc {
    uint64_t struct_size;
    int32_t plan_kind, elem, source, transform;
    const void *plan;
    const void *x, *x2;
    void *out;
    int64_t T, ldx, ldo, out_pstride;
    int32_t layout, out_layout;
    double offset;
    int32_t pow_first, n_pow;
    const double *thresholds;
    int32_t n_thr, flags;
    int32_t ksplit, n_plans;
    const int32_t *devices;
    const int64_t *rows;
    void *group;
    int32_t root, reserved0;
    void *stream;
} wagg_apply_desc;
int wagg_apply(const wagg_apply_desc *desc);

/* ---- many-plans: several weightings and nested levels of one table, one pass over X (0.5.0) ---------------------------
 * wagg_plan_create_many builds ONE plan for n_weights weight columns of the same segment table (w_eff[k]: nseg values each,
 * backup-filled as for wagg_plan_create) and n_levels coarse levels derived from the fine one (level_code[l]: nseg coarse
 * codes in [0, level_R[l]), < 0 = null label).  Limits: 1 <= n_weights <= 4, 0 <= n_levels <= 3.
 *   kept rows  a row is kept if any weighting keeps it; a weighting whose w_eff is NaN on a kept row gives it weight 0 (S6)
 *   nesting    over the rows with some weight that is not NaN: the fine code is null iff the coarse one is, and every fine
 *              code maps to exactly one coarse code -- else WAGG_EINVAL naming the first offending row.  Every check runs
 *              before any device call.
 *   den        level 0 (fine): per weighting, what wagg_plan_create of that column gives; coarse levels: fp64 sums in row
 *              order, bit for bit wagg_plan_get_den of a wagg_plan_create over the coarse codes.
 * The result of an apply concatenates every plane along the region axis, level-major, then weighting: plane (l, k) takes
 * columns [off(l, k), off(l, k) + R_l) of a (time, region) result (rows of a (region, time) one), R_0 = R, off(l, k) =
 * sum of n_weights * R_j over j < l, plus k * R_l.  wagg_plan_get_info's R is that width (out_cols), which ldo must reach.
 * wagg_apply takes a many-plan as plan_kind WAGG_PLAN_SEGMENT with source WAGG_SRC_DEVICE or WAGG_SRC_HOST (one crossing of
 * PCIe for all planes; WAGG_HOST_LINES as for a single plan) and transform WAGG_XF_NONE; anything else is WAGG_EUNSUPPORTED.
 * (time, gridcell) data on a plan with a whole-line chunking for the element type reads X once for all weightings (fp32: up
 * to four per pass, fp64: two) and derives the coarse levels from the fine partial sums; fine planes are bit for bit the
 * results of single plans over the same kept rows.  Other layouts / plans run the single-plan kernels once per weighting, and
 * derived levels there are WAGG_EUNSUPPORTED.                                                                                    */
int wagg_plan_create_many(const int32_t *cell_idx, const int32_t *region_code, const double *const *w_eff, int n_weights,
                          int64_t nseg, int64_t G, int32_t R, int64_t row_len, const int32_t *const *level_code,
                          const int32_t *level_R, int n_levels, int flags, wagg_plan **out);
/* n_weights = n_levels = 0 for a plan of wagg_plan_create; level_R: n_levels values (may be NULL); out_cols: result width */
int wagg_plan_many_info(const wagg_plan *plan, int *n_weights, int *n_levels, int32_t *level_R, int64_t *out_cols);
int wagg_plan_get_den_many(const wagg_plan *plan, int weighting, int level, double *den_host /* R_level values */);

/* ---- period totals: sums over the rows of a (T, n) device matrix, per period (0.6.0) ------------------------------------
 * out[k][p][j] = sum over the rows t of period p, IN LIST ORDER, of f_k(X[t, j])  -- the degree-day measures as the
 * reference defines them (EDD_P = sum of EDD_d over the days of P, transformations.py:17-19), annual or monthly totals of
 * any aggregate.  The sum is linear, so it may run in front of an apply (on the field: X = the (T, G) field, n = G, f = the
 * transform) or behind it (X = the (T, R) result, n = R, no transform, WAGG_PERIOD_KEEP_NAN).
 *   X_dev, X2_dev   row-major (T, n), leading dimension ldx >= n; X2_dev (tasmax) only with WAGG_XF_EDD
 *   row_begin_dev   P + 1 ascending int32 offsets into rows_dev (n_rows entries): period p owns rows_dev[row_begin[p] ..
 *   rows_dev        row_begin[p + 1]).  Rows in any order; a row may be listed in no period (a dropped 29 February) or in
 *                   several; an empty period totals 0
 *   transform       WAGG_XF_NONE (one plane); WAGG_XF_POLY: (x + offset)^q, q = pow_first .. pow_first + n_pow - 1, n_pow <= 4,
 *                   q <= 16; WAGG_XF_EDD: snyder_edd(x + offset, x2 + offset, thresholds[k]) (host array), n_thr <= 4 -- the
 *                   device functions of the fused applies, evaluated in the element type
 *   out_dev         plane k at out_dev + k * out_pstride, row p at + p * ldo (ldo >= n, out_pstride >= P * ldo)
 *   status_dev      one device int32, OR-ed with 1 when a transformed value was +-inf (an inf in X, a power that overflows);
 *                   the caller zeroes it.  Sums of +inf and -inf over DIFFERENT days of a cell differ between the two
 *                   orders (NaN in front of an apply, per-day handling behind it): a caller who needs the daily semantics
 *                   redoes such a call behind the apply
 *   work_dev        optional scratch of work_bytes bytes: when n * P is too small to fill the device a period's list is cut
 *                   into consecutive parts whose fp64 partial sums land here and are added in part order by a second launch
 *                   (wagg_period_reduce_work_bytes says how much that takes; NULL / less: fewer parts or one)
 *   flags           WAGG_PERIOD_KEEP_NAN: NaN propagates (for (T, R) results: a region without weight stays NaN); without
 *                   it a NaN f_k counts 0 (S6: the NaN product leaves the numerator, its weight stays in the denominator).
 *                   WAGG_PERIOD_ROWS_CHECKED: the caller vouches for the lists; without it they are checked on the device
 *                   first (row_begin ascending within [0, n_rows], every row in [0, T), else WAGG_EINVAL), which BLOCKS on
 *                   `stream`.  With it the call is asynchronous; a row index outside [0, T) is skipped, never read.
 * fp32 and fp64 data both accumulate in fp64 and are rounded once; list order, no atomics on a sum: bit-reproducible.   */
#define WAGG_PERIOD_KEEP_NAN 1
#define WAGG_PERIOD_ROWS_CHECKED 2
int wagg_period_reduce_f32(const float *X_dev, const float *X2_dev, int64_t T, int64_t n, int64_t ldx,
                           const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows, int transform,
                           double offset, int pow_first, int n_pow, const double *thresholds, int n_thr, int flags,
                           float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                           int64_t work_bytes, void *stream);
int wagg_period_reduce_f64(const double *X_dev, const double *X2_dev, int64_t T, int64_t n, int64_t ldx,
                           const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows, int transform,
                           double offset, int pow_first, int n_pow, const double *thresholds, int n_thr, int flags,
                           double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                           int64_t work_bytes, void *stream);
int64_t wagg_period_reduce_work_bytes(int64_t n, int32_t P, int64_t n_rows, int planes);

/* ---- growing-season totals: the period sum with a day-of-year window per cell (0.7.0) ---------------------------------------
 * out[k][p][j] = sum over the rows t of period p, IN LIST ORDER, on which cell j is in season, of f_k(X[t, j]) -- the
 * reference's growing-season mask (utils.py:83-153) times the daily field, summed over time in front of an apply.  The
 * arguments are those of wagg_period_reduce_* plus
 *   doy_dev   T int32: the day of year of every row of X (1..366); a value outside 0..1023 is in no season
 *   win_dev   n int32: one packed window per cell.  Bits 0-9: a (first day), bits 10-19: b (last day), bit 20
 *             (WAGG_SEASON_INVERT): the season is the complement of [a, b] (it wraps the year end; a and b themselves are then
 *             out of season), bit 21 (WAGG_SEASON_NULL): never in season (no planting day; the mask value is NaN).  Cell j is in
 *             season on day d iff not null and (a <= d <= b) != invert.  An empty interval is stored as a = 1, b = 0.
 * A value out of season is selected away, never multiplied: NaN or +-inf there reaches neither a sum nor status_dev, and a
 * piece of a row none of whose cells is in season is not read.  NaN in season counts 0 (S6); there is no keep-NaN form
 * (flags: WAGG_PERIOD_ROWS_CHECKED only).  status_dev bit 0: an IN-SEASON transformed value was +-inf.  With every window
 * open all year (a = 0, b = 1023) the result is bit for bit that of wagg_period_reduce_*.
 * wagg_season_mask writes the mask itself: out_dev[j * T + t] = NaN (null window), 1 or 0 -- (n, T) row-major, fp64.          */
#define WAGG_SEASON_INVERT (1 << 20)
#define WAGG_SEASON_NULL (1 << 21)
int wagg_season_reduce_f32(const float *X_dev, const float *X2_dev, int64_t T, int64_t n, int64_t ldx,
                           const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                           const int32_t *doy_dev, const int32_t *win_dev, int transform, double offset, int pow_first, int n_pow,
                           const double *thresholds, int n_thr, int flags, float *out_dev, int64_t ldo, int64_t out_pstride,
                           int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int wagg_season_reduce_f64(const double *X_dev, const double *X2_dev, int64_t T, int64_t n, int64_t ldx,
                           const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                           const int32_t *doy_dev, const int32_t *win_dev, int transform, double offset, int pow_first, int n_pow,
                           const double *thresholds, int n_thr, int flags, double *out_dev, int64_t ldo, int64_t out_pstride,
                           int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int64_t wagg_season_reduce_work_bytes(int64_t n, int32_t P, int64_t n_rows, int planes);
int wagg_season_mask(const int32_t *doy_dev, int64_t T, const int32_t *win_dev, int64_t n, double *out_dev /* [n][T] */, void *stream);

/* ---- degree-day ladders: Snyder degree days at every reference temperature in one pass (0.8.0) -----------------------------
 * out[k][p][j] = sum over the rows t of period p, IN LIST ORDER, on which cell j is in season, of
 * snyder_edd(tasmin[t, j] + offset, tasmax[t, j] + offset, thresholds[k]),  k = 0 .. n_thr - 1,  1 <= n_thr <= WAGG_EDD_LADDER_MAX
 * -- wagg_season_reduce_* with WAGG_XF_EDD without its cap of four thresholds: one launch, the thresholds taken in groups of
 * WAGG_EDD_LADDER_GROUP.  Arguments as there (tasmin_dev / tasmax_dev: row-major (T, n), one leading dimension ldx), except
 *   doy_dev, win_dev   both NULL: no season, every listed row counts (wagg_period_reduce_* with WAGG_XF_EDD); one of them NULL
 *                      alone is WAGG_EINVAL
 *   thresholds         n_thr host doubles, converted to the element type
 *   flags              WAGG_PERIOD_ROWS_CHECKED only (no keep-NaN form: a NaN term counts 0, S6)
 *   out_dev            plane k at out_dev + k * out_pstride, row p at + p * ldo (out_pstride >= P * ldo when n_thr > 1)
 *   work_dev           wagg_edd_ladder_work_bytes(n, P, n_rows, n_thr) bytes: n_thr / planes times what
 *                      wagg_season_reduce_work_bytes reports for `planes` (equal to it up to four thresholds)
 * status_dev bit 0: an in-season value was +-inf; a value out of season is never looked at.  Per threshold and row a wave
 * evaluates the band expression only if a lane's in-season cells span the threshold (least tasmin < threshold < greatest
 * tasmax: no cell whose sinusoid crosses it escapes that); the value is the one the four-plane kernels select.  BIT-EQUALITY: when every call gets the workspace its own *_work_bytes reports, plane k is
 * bit for bit the plane wagg_season_reduce_* gives for thresholds[k] (in whichever group of up to four it is called there),
 * and with doy_dev = win_dev = NULL the plane wagg_period_reduce_* gives.                                                     */
#define WAGG_EDD_LADDER_MAX 64
#define WAGG_EDD_LADDER_GROUP 8
int wagg_edd_ladder_reduce_f32(const float *tasmin_dev, const float *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                               const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                               const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *thresholds, int n_thr,
                               int flags, float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                               int64_t work_bytes, void *stream);
int wagg_edd_ladder_reduce_f64(const double *tasmin_dev, const double *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                               const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                               const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *thresholds, int n_thr,
                               int flags, double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                               int64_t work_bytes, void *stream);
int64_t wagg_edd_ladder_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_thr);

/* ---- temperature bins: the days a cell spends in each bin, per period and season, in one pass (0.10.0) ------------------------
 * out[k][p][j] = the number of rows t of period p's list on which cell j is in season and
 * edges[k] <= X[t, j] + offset < edges[k + 1],  k = 0 .. n_edges - 2,  2 <= n_edges <= WAGG_BIN_EDGES_MAX (64 bins) -- one
 * launch, the bins taken in groups of WAGG_BIN_GROUP.  Arguments as for wagg_edd_ladder_reduce_* with ONE field, except
 *   edges              n_edges host doubles, strictly ascending; -inf may come first and +inf last (open end bins); a NaN edge,
 *                      equal or descending edges are WAGG_EINVAL
 *   offset             finite; the edges are in the units of X + offset (degrees C for a Kelvin field with offset -273.15)
 *   flags              WAGG_PERIOD_ROWS_CHECKED only
 *   out_dev            plane k (a bin) at out_dev + k * out_pstride, row p at + p * ldo (out_pstride >= P * ldo when n_edges > 2);
 *                      the count as a value of the element type, exact in fp32 up to 2^24 days
 *   work_dev           wagg_bin_days_work_bytes(n, P, n_rows, n_edges) bytes: what wagg_period_reduce_work_bytes reports for
 *                      n_edges - 1 planes
 * THE COMPARISON RULE: nothing is shifted in the element type.  The host forms c_k = edges[k] - offset in fp64 and the kernel
 * compares the RAW X[t, j] against ceilT(c_k), the smallest value of the element type that is not below c_k (fp32: (float)c_k,
 * stepped up once by nextafterf if that lies below c_k; infinities pass through).  For every representable x, x >= ceilT(c)
 * holds exactly when (double)x >= c: an fp32 field is binned as its exact values would be in fp64, a value equal to an edge
 * lands in the upper bin, and no value near an edge can flip.
 * NaN is in no bin (S6: it counts 0).  -inf lands in a first bin that is open below (edges[0] = -inf) and nowhere else, +inf in
 * no bin; an IN-SEASON +-inf sets bit 0 of status_dev.  A value out of season is never counted and sets no status; a piece
 * none of whose cells is in season is not read.  Counts are integers: every split of a list, and every run, gives the same bits. */
#define WAGG_BIN_EDGES_MAX 65
#define WAGG_BIN_GROUP 8
int wagg_bin_days_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                             const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                             double offset, const double *edges, int n_edges, int flags, float *out_dev, int64_t ldo,
                             int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int wagg_bin_days_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                             const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                             double offset, const double *edges, int n_edges, int flags, double *out_dev, int64_t ldo,
                             int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int64_t wagg_bin_days_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_edges);

/* ---- hinges: truncated powers of the daily value about a knot, per period and season, in one pass (0.11.0) --------------------
 * out[j][p][i] = sum over the rows t of period p, IN LIST ORDER, on which cell i is in season, of
 * h(X[t, i]; knots[j]),  h(x; k) = max(+-((x + offset) - k), 0)^power,  j = 0 .. n_knots - 1,  1 <= n_knots <= WAGG_HINGE_MAX --
 * one launch, the knots taken in groups of WAGG_HINGE_GROUP.  power 1 on a daily mean: cooling (WAGG_HINGE_ABOVE) / heating
 * (WAGG_HINGE_BELOW) degree days; power 1 at several knots: a linear spline; power 3: the terms of a restricted cubic spline.
 * Arguments as for wagg_bin_days_reduce_*, except
 *   knots              n_knots finite host doubles in any order, converted to the element type; in the units of X + offset
 *   power              1..3;  side: WAGG_HINGE_ABOVE (+) or WAGG_HINGE_BELOW (-)
 *   tail_knots, tail_a, tail_b   all NULL: no tail.  Otherwise two finite knots kA, kB and n_knots finite coefficients each: plane
 *                      j leaves the kernel as (S_j + tail_a[j] * S_A) + tail_b[j] * S_B, S_A / S_B being the same sums at kA / kB
 *                      -- formed in fp64, per part of a split list, before the cast to the element type (the restricted cubic
 *                      spline's cancellation beyond its last knot then happens among fp64 sums)
 *   flags              WAGG_PERIOD_ROWS_CHECKED only (no keep-NaN form)
 *   out_dev            plane j (a knot) at out_dev + j * out_pstride, row p at + p * ldo (out_pstride >= P * ldo when n_knots > 1)
 *   work_dev           wagg_hinge_work_bytes(n, P, n_rows, n_knots) bytes: what wagg_bin_days_work_bytes reports for as many planes
 * THE ARITHMETIC: d = (X[t, i] + offset) - knot in the element type, in exactly these two roundings (offset and knot converted
 * to the element type first; nothing is contracted), negated for WAGG_HINGE_BELOW; the term is d > 0 ? d^power : 0 with
 * d^2 = d * d and d^3 = (d * d) * d in the element type; sums are fp64.  An fp32 Kelvin field carries up to one ulp of the
 * Kelvin value (3e-5 K) into d -- unlike the bins' exact comparison.  NaN gives 0 (S6).  An IN-SEASON +-inf of the field sets
 * bit 0 of status_dev, whichever side is asked for; a value out of season reaches neither a sum nor the status word; a piece
 * none of whose cells is in season is not read.  BIT-EQUALITY: when every call gets the workspace its own wagg_hinge_work_bytes
 * reports, plane j of a many-knot call is bit for bit the plane of the call with knots[j] (and its coefficients) alone, and an
 * all-year window for every cell gives the bits of the call with doy_dev = win_dev = NULL.                                      */
#define WAGG_HINGE_MAX 64
#define WAGG_HINGE_GROUP 8
#define WAGG_HINGE_ABOVE 0
#define WAGG_HINGE_BELOW 1
int wagg_hinge_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                          const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                          double offset, const double *knots, int n_knots, int power, int side, const double *tail_knots,
                          const double *tail_a, const double *tail_b, int flags, float *out_dev, int64_t ldo, int64_t out_pstride,
                          int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int wagg_hinge_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                          const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                          double offset, const double *knots, int n_knots, int power, int side, const double *tail_knots,
                          const double *tail_a, const double *tail_b, int flags, double *out_dev, int64_t ldo, int64_t out_pstride,
                          int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int64_t wagg_hinge_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_knots);

/* ---- sinusoid exposure bins: the time a day's temperature curve spends in each bin, per period and season (0.12.0) -------------
 * out[k][p][j] = sum over the rows t of period p, IN LIST ORDER, on which cell j is in season, of
 * A(lo, hi, edges[k]) - A(lo, hi, edges[k + 1]),  lo = tasmin[t, j] + offset, hi = tasmax[t, j] + offset (shifted in the element
 * type, as the ladder shifts them),  k = 0 .. n_edges - 2,  2 <= n_edges <= WAGG_EXPOSURE_EDGES_MAX (64 bins) -- one launch, the
 * bins taken in groups of WAGG_EXPOSURE_GROUP.  A is the fraction of the day the single-sine curve of snyder_edd spends above
 * e = edges[k] converted to the element type, A = -d EDD / de:
 *   0                          if lo or hi is NaN   (the day is in no bin; checked first)
 *   1                          if !(lo < e)         (snyder_edd's own comparisons, in its order)
 *   0                          if !(hi > e)
 *   clamp(acos(z) / pi, 0, 1)  otherwise,  z = (e - M) / w clamped to [-1, 1],  M = (hi + lo) / 2,  w = (hi - lo) / 2
 * The outer cases are exactly 1 and 0; e = -inf gives 1 for every day without NaN, e = +inf gives 0; tasmin > tasmax is a step
 * at tasmin.  fp32 evaluates acos(z) / pi as sqrt(t) Q(t), t = 1 - |z| = min(hi - e, e - lo) / w, with a fitted Q (<= 1.5e-7
 * from the fp64 libm value of the same lo, hi, e); fp64 calls libm.  The per-day difference is formed in the element type,
 * sums are fp64.  Arguments as for wagg_edd_ladder_reduce_* with (edges, n_edges) in place of (thresholds, n_thr):
 *   edges              n_edges host doubles, strictly ascending; -inf may come first and +inf last (open end bins); a NaN edge,
 *                      equal or descending edges are WAGG_EINVAL
 *   offset             finite
 *   flags              WAGG_PERIOD_ROWS_CHECKED only (no keep-NaN form)
 *   out_dev            plane k (a bin) at out_dev + k * out_pstride, row p at + p * ldo (out_pstride >= P * ldo when n_edges > 2)
 *   work_dev           wagg_exposure_work_bytes(n, P, n_rows, n_edges) bytes: what wagg_period_reduce_work_bytes reports for
 *                      n_edges - 1 planes.  Without it a period's list is summed in one part.
 * An IN-SEASON +-inf in either field sets bit 0 of status_dev (its bins are then unspecified but finite); a value out of season
 * reaches neither a sum nor the status word; a piece none of whose cells is in season is not read.  Per edge and row a wave
 * evaluates the arccosine only if a lane's in-season cells span the edge; the value is the one the full function selects, so a
 * column's bins do not depend on its neighbours.                                                                              */
#define WAGG_EXPOSURE_EDGES_MAX 65
#define WAGG_EXPOSURE_GROUP 8
int wagg_exposure_reduce_f32(const float *tasmin_dev, const float *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                             const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                             const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *edges, int n_edges,
                             int flags, float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                             int64_t work_bytes, void *stream);
int wagg_exposure_reduce_f64(const double *tasmin_dev, const double *tasmax_dev, int64_t T, int64_t n, int64_t ldx,
                             const int32_t *row_begin_dev, const int32_t *rows_dev, int32_t P, int64_t n_rows,
                             const int32_t *doy_dev, const int32_t *win_dev, double offset, const double *edges, int n_edges,
                             int flags, double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                             int64_t work_bytes, void *stream);
int64_t wagg_exposure_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_edges);

/* ---- spells: runs of consecutive days past a threshold, per period and season, in one pass (0.13.0) ---------------------------
 * Heat-wave / cold-spell days, the number of such events and the longest run, for thresholds[k],  k = 0 .. n_thr - 1,
 * 1 <= n_thr <= WAGG_SPELL_MAX -- one launch, the thresholds taken in groups of WAGG_SPELL_GROUP.  The one statistic of the
 * row-list families in which a day's contribution depends on its neighbours.  Cell j, period p, threshold k: the entries i of
 * rows[row_begin[p] : row_begin[p + 1]] are walked IN LIST ORDER.  Entry i is HOT when t = rows[i] lies in [0, T), cell j is in
 * season on doy[t] (when a season is given) and  X[t, j] + offset >= thresholds[k]  (below = 0)  or  < thresholds[k]  (below = 1).
 * A RUN is a maximal stretch of hot entries i, i + 1, ... with rows[i + 1] == rows[i] + 1.  A gap in the row numbers (a dropped
 * row, another January of a month-of-all-years labelling), an out-of-season day, a NaN and the end of the period's list all end
 * the run: RUNS ARE TRUNCATED AT PERIOD BOUNDARIES, a heat wave over New Year's Eve is one run in each of the two years.  With
 * L = min_length, out[k][p][j] is
 *   WAGG_SPELL_DAYS      the number of hot entries that belong to runs of length >= L
 *   WAGG_SPELL_EVENTS    the number of runs of length >= L
 *   WAGG_SPELL_LONGEST   the length of the longest run (min_length is not used and must be 1)
 * Arguments as for wagg_bin_days_reduce_*, except
 *   thresholds         n_thr finite host doubles in any order, duplicates allowed (the planes are independent); NaN or +-inf
 *                      (a constant plane) is WAGG_EINVAL; in the units of X + offset
 *   min_length         1..WAGG_SPELL_MIN_LENGTH_MAX;  stat: one of the three above;  below: 0 or 1
 *   out_dev            plane k (a threshold) at out_dev + k * out_pstride, row p at + p * ldo (out_pstride >= P * ldo when
 *                      n_thr > 1); the count as a value of the element type, exact in fp32 up to 2^24
 *   work_dev, work_bytes   IGNORED.  A run does not add across the parts of a list, so this family never splits one:
 *                      wagg_spell_work_bytes is 0.  (Combining parts through prefix / suffix / interior runs is not built; a
 *                      single long period on a packed row therefore fills fewer blocks than the other families' launches.)
 * THE COMPARISON RULE is the bins': the kernel compares the RAW X[t, j] against ceilT(thresholds[k] - offset), the difference
 * formed in fp64, so an fp32 Kelvin field is classified as its exact values would be in fp64 -- x >= ceilT(c) exactly when
 * (double)x >= c, and x < ceilT(c) exactly when (double)x < c.  NaN is never hot, on either side.  An IN-SEASON +-inf, hot or not,
 * sets bit 0 of status_dev; a value out of season is cold and sets no status; a piece none of whose cells is in season is not
 * read but still ends the runs.  Counts are integers: every run gives the same bits, and plane k of a many-threshold call is
 * the plane of the call with thresholds[k] alone.                                                                              */
#define WAGG_SPELL_MAX 64
#define WAGG_SPELL_GROUP 8
#define WAGG_SPELL_MIN_LENGTH_MAX 32767
#define WAGG_SPELL_DAYS 0
#define WAGG_SPELL_EVENTS 1
#define WAGG_SPELL_LONGEST 2
int wagg_spell_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                          const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                          double offset, const double *thresholds, int n_thr, int min_length, int stat, int below, int flags,
                          float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes,
                          void *stream);
int wagg_spell_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                          const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                          double offset, const double *thresholds, int n_thr, int min_length, int stat, int below, int flags,
                          double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes,
                          void *stream);
int64_t wagg_spell_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_thr);

/* ---- spells that run across period boundaries (0.18.0) -----------------------------------------------------------------------
 * wagg_spell_reduce_*'s three statistics with the runs NOT truncated at the end of a period's list: CDD / CWD (the longest dry
 * / wet spell, defined on spells that run through New Year), a December-January heat wave with min_length = 6, every month
 * end of a monthly call.  The argument list, the constants (WAGG_SPELL_*), the comparison rule, the season and the status word
 * are wagg_spell_reduce_*'s; wagg_spell_span_work_bytes is 0 and work_dev / work_bytes are ignored.  THE DEFINITION:
 * The CHAIN is the concatenation of the periods' lists in period order: the entries rows[row_begin[0] : row_begin[P]], row_begin
 * confined to [0, n_rows] and made ascending as wagg_spell_reduce_* confines it.  For cell j and threshold k:
 *   HOT     entry i is hot exactly as in wagg_spell_reduce_*: t = rows[i] lies in [0, T), cell j is in season on doy[t] (when a
 *           season is given) and the raw X[t, j] passes against ceilT(thresholds[k] - offset).  NaN is never hot.
 *   JOINS   entry i joins entry i - 1 when rows[i] == rows[i - 1] + 1.  It does not matter whether a period boundary, or several
 *           empty periods, lie between them: empty lists are transparent.
 *   RUN     a maximal stretch of hot, joined entries of the chain.
 *   r_i     the RUNNING LENGTH at entry i: its position within its run, starting at 1, or 0 when cold.  It is carried over
 *           boundaries.
 *   l       the run's WHOLE LENGTH.
 * With L = min_length, out[k][p][j] is
 *   WAGG_SPELL_DAYS      the hot entries of p's list whose run has l >= L.  Every day is counted in its own period; whether it
 *                        counts is decided by the whole run.
 *   WAGG_SPELL_EVENTS    the entries of p's list with r_i == L.  A run counts once, in the period in which it reaches
 *                        min_length; for L = 1 that is the period in which it starts.
 *   WAGG_SPELL_LONGEST   the greatest r_i over the entries of p's list, and 0 for an empty list.  A spell counts in a period for
 *                        as long as it has lasted by then, reaching back to its start wherever that lies: a year wholly inside
 *                        one dry spell reports at least its own length, a spell from 20 December to 10 January gives 12 and 22.
 *                        min_length must be 1.
 * THE LAWS that follow: where no run crosses a boundary, all three equal wagg_spell_reduce_* bit for bit; the sum over p of DAYS
 * and of EVENTS, and the greatest LONGEST over p, equal wagg_spell_reduce_*'s single-period result on the chain taken as one
 * list; LONGEST is never below the truncating value.  Joins are found only between neighbours in the chain, so the mode means
 * something for periods whose lists follow each other in time (years, months, ascending labels); with labels that pool the
 * Januaries of all years nothing joins across lists and the result is wagg_spell_reduce_*'s.
 * One launch of column block x threshold group blocks -- NO period dimension: a block walks the whole record in order, which is
 * the cost of the mode (csrc/wagg_spells_span.hip).  DAYS credits the days of a run that lie in earlier periods by a
 * read-modify-write of what the same thread stored there in this launch: no atomics, no scratch, nothing read from out_dev that
 * the launch did not write; stream-ordered and capturable.  tests/spell_span_ref.py is the NumPy restatement.  (The names carry no
 * _reduce: every wagg_*_reduce_f32 / _f64 export is a family of tests/rowlist_layout.py's case table; this call's pitched and
 * poisoned out_dev is checked in tests/test_gpu_spell_span.py.)                                                                  */
int wagg_spell_span_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                               const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                               double offset, const double *thresholds, int n_thr, int min_length, int stat, int below, int flags,
                               float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                               int64_t work_bytes, void *stream);
int wagg_spell_span_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                               const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                               double offset, const double *thresholds, int n_thr, int min_length, int stat, int below, int flags,
                               double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                               int64_t work_bytes, void *stream);
int64_t wagg_spell_span_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_thr);

/* ---- rolling-window extremes: the greatest / least running sum or mean over W days, per period and season (0.14.0) -------------
 * TXx / TNn (W = 1), the hottest or coldest N-day mean, Rx1day / Rx5day: the extreme over a period of the sum (or mean) of W
 * consecutive days, for windows[k] days,  k = 0 .. n_win - 1,  1 <= n_win <= WAGG_ROLL_MAX_WINDOWS,  1 <= windows[k] <=
 * WAGG_ROLL_WINDOW_MAX -- one launch, the field read once (WAGG_ROLL_GROUP windows a block).  Cell j, period p, window length W:
 * the entries i of rows[row_begin[p] : row_begin[p + 1]] are walked IN LIST ORDER.  Entry i is VALID when t = rows[i] lies in
 * [0, T), cell j is in season on doy[t] (when a season is given) and X[t, j] is not NaN.  A WINDOW of length W ends at entry i when
 * the entries i - W + 1 .. i all lie in this period's list, rows[m + 1] == rows[m] + 1 along them, and all are valid.  A gap in
 * the row numbers, an out-of-season day, a NaN and the start of the list invalidate every window that would hold them: WINDOWS
 * NEVER REACH ACROSS A PERIOD BOUNDARY, a 5-day window ending on 2 January does not exist in the new year.  The window's sum is
 * formed in fp64 from the raw elements, newest to oldest:  s = ((x[i] + x[i-1]) + x[i-2]) + ... + x[i-W+1].
 *   WAGG_ROLL_MAX   m = -inf, then  m = s > m ? s : m  over the windows in list order;   WAGG_ROLL_MIN   +inf and <
 *   WAGG_ROLL_MEAN  out[k][p][j] = (T)(m / (double)W + offset)        (division is monotone: the extreme of the means)
 *   WAGG_ROLL_SUM   out[k][p][j] = (T)(m + (double)W * offset)        (the product formed on the host)
 * one rounding from fp64 to the element type.  A period WITHOUT A VALID WINDOW for a cell (an empty list, one shorter than W,
 * all gaps / out of season / NaN) gives NaN for that cell and window.
 * Arguments as for wagg_spell_reduce_*, except
 *   windows            n_win host int32 in 1..WAGG_ROLL_WINDOW_MAX, any order, duplicates allowed; plane k of out_dev is windows[k]
 *   stat, of           WAGG_ROLL_MAX / _MIN, WAGG_ROLL_MEAN / _SUM; offset finite
 *   work_dev, work_bytes   IGNORED.  A window does not add across the parts of a list, so this family never splits one:
 *                      wagg_rolling_work_bytes is 0.
 * An IN-SEASON +-inf sets bit 0 of status_dev; a value out of season is never looked at; a piece none of whose cells is in
 * season is not read but still invalidates the windows over that day.  Every run gives the same bits, plane k of a many-window
 * call is the plane of the call with windows[k] alone, and the results equal a NumPy restatement exactly (tests/rolling_ref.py). */
#define WAGG_ROLL_WINDOW_MAX 16
#define WAGG_ROLL_MAX_WINDOWS 8
#define WAGG_ROLL_GROUP 8
#define WAGG_ROLL_MAX 0
#define WAGG_ROLL_MIN 1
#define WAGG_ROLL_MEAN 0
#define WAGG_ROLL_SUM 1
int wagg_rolling_reduce_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                            const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                            double offset, const int32_t *windows, int n_win, int stat, int of, int flags, float *out_dev, int64_t ldo,
                            int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int wagg_rolling_reduce_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                            const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                            double offset, const int32_t *windows, int n_win, int stat, int of, int flags, double *out_dev, int64_t ldo,
                            int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int64_t wagg_rolling_work_bytes(int64_t n, int32_t P, int64_t n_rows, int n_win);

/* ---- period quantiles: per-cell order statistics of the daily values of a period and season (0.15.0) --------------------------
 * The median, the 5th / 95th / 99th percentile, R95p thresholds: for q[k],  k = 0 .. n_q - 1,  1 <= n_q <= WAGG_QUANT_MAX, in one
 * launch.  Cell j, period p, the entries i of rows[row_begin[p] : row_begin[p + 1]]: entry i is VALID when t = rows[i] lies in
 * [0, T), cell j is in season on doy[t] (when a season is given) and X[t, j] is not NaN.  Order and gaps do not matter, a row
 * listed twice counts twice, an in-season +-inf is valid (and sets bit 0 of status_dev).  Let m be the number of valid entries
 * and v[0] <= ... <= v[m - 1] their raw elements sorted (-0.0 ahead of +0.0: equal as numbers).  For every q[k]:
 *   h = (double)(m - 1) * q[k]   (one fp64 product),   lo = (int)floor(h),   g = h - (double)lo
 *   WAGG_QUANT_LINEAR   r = g == 0 ? (double)v[lo] : (double)v[lo] + ((double)v[lo + 1] - (double)v[lo]) * g
 *                       (difference, product and sum each rounded: no fused multiply-add)
 *   WAGG_QUANT_LOWER    r = v[lo]
 *   WAGG_QUANT_HIGHER   r = v[g == 0 ? lo : lo + 1]
 *   out[k][p][j] = (T)(r + offset), rounded once;  m == 0 gives NaN.
 * Arguments as for wagg_rolling_reduce_*, except
 *   q, n_q             n_q host doubles in [0, 1], any order, duplicates allowed; plane k of out_dev is q[k]
 *   method             WAGG_QUANT_LINEAR / _LOWER / _HIGHER; offset finite
 *   max_rows           1 .. WAGG_QUANT_ROWS_MAX: the caller's bound on the longest list; a block holds its period's whole list in
 *                      128 * max_rows bytes of LDS.  Without WAGG_PERIOD_ROWS_CHECKED the blocking look at the lists also
 *                      rejects a list longer than max_rows (WAGG_EINVAL).  With the flag the kernel confines itself: a period
 *                      whose list is longer writes NaN in every plane and sets bit 1 of status_dev.
 *   work_dev, work_bytes   IGNORED.  An order statistic does not add across the parts of a list, so a list is never split;
 *                      there is no *_work_bytes.
 * Every bad argument is WAGG_EINVAL with a message, decided before any device call.  A value out of season is never looked at.
 * The selection is exact: the results equal a NumPy restatement bit for bit (tests/quantile_ref.py), plane k of a many-quantile
 * call is the plane of the call with q[k] alone, and q = 1 / q = 0 are wagg_rolling_reduce_*'s W = 1 maximum / minimum. */
#define WAGG_QUANT_MAX 16
#define WAGG_QUANT_ROWS_MAX 1024
#define WAGG_QUANT_LINEAR 0
#define WAGG_QUANT_LOWER 1
#define WAGG_QUANT_HIGHER 2
int wagg_quantile_select_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                             const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                             double offset, const double *q, int n_q, int method, int32_t max_rows, int flags, float *out_dev,
                             int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);
int wagg_quantile_select_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                             const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                             double offset, const double *q, int n_q, int method, int32_t max_rows, int flags, double *out_dev,
                             int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes, void *stream);

/* ---- spells and exceedances against PER-CELL thresholds, per period and season, in one pass (0.16.0) ----------------------------
 * Days above the cell's own 90th percentile (TX90p / TN10p), warm-spell days (WSDI / CSDI), events above the local 95th percentile,
 * precipitation on days above the cell's 95th wet-day percentile (R95pTOT): wagg_spell_reduce_*'s statistics with the threshold
 * read from a device field -- what wagg_quantile_select_* writes, or a caller's baseline -- for n_thr threshold levels,
 * 1 <= n_thr <= WAGG_CELL_SPELL_MAX, in one launch, taken in groups of WAGG_CELL_SPELL_GROUP.
 *   thr_dev            a DEVICE array of the element type, logically (n_thr, M, n):  thr[k][m][j] = thr_dev[k * thr_kstride +
 *                      m * ldt + j];  ldt >= n, thr_kstride >= M * ldt, M >= 1.  Read once per block, ahead of the rows.
 *   plane_of_period_dev   a DEVICE int32[P]: period p reads the ONE plane m = plane_of_period_dev[p] (a plane per ROW -- calendar-day
 *                      thresholds inside a period -- is wagg_row_cell_spells_*, below).  NULL is allowed only for
 *                      M == 1 (m = 0) and M == P (m = p); otherwise WAGG_EINVAL.  Without WAGG_PERIOD_ROWS_CHECKED the library's
 *                      blocking look at the lists also checks 0 <= m < M (WAGG_EINVAL).  With the flag the kernel confines itself:
 *                      a period whose m is out of range writes NaN in every plane and sets bit 2 of status_dev.
 * Cell j, period p, level k: the entries i of rows[row_begin[p] : row_begin[p + 1]] are walked IN LIST ORDER.  Entry i is HOT when
 * t = rows[i] lies in [0, T), cell j is in season on doy[t] (when a season is given) and  X[t, j] + offset >= thr[k][m][j]
 * (below = 0)  or  < thr[k][m][j]  (below = 1).  THE COMPARISON RULE is wagg_spell_reduce_*'s, formed on the device: the kernel
 * compares the RAW X[t, j] against  c = ceilT((double)thr[k][m][j] - offset)  -- one fp64 subtraction, rounded to nearest, stepped
 * up once where that lies below -- so a threshold field that is constant over the cells gives wagg_spell_reduce_*'s plane BIT FOR
 * BIT.  NaN days are never hot; +-inf thresholds compare as they compare (a constant plane is allowed here).  A NaN THRESHOLD MAKES
 * out[k][p][j] NaN, for every statistic.  Runs, gaps, seasons and bit 0 of status_dev are wagg_spell_reduce_*'s: a gap in the row
 * numbers, an out-of-season day, a NaN and the end of the list end a run, RUNS ARE TRUNCATED AT PERIOD BOUNDARIES, an in-season
 * +-inf sets bit 0, a piece none of whose cells is in season is not read but still ends the runs.  With L = min_length, out[k][p][j] is
 *   WAGG_SPELL_DAYS / WAGG_SPELL_EVENTS / WAGG_SPELL_LONGEST     as for wagg_spell_reduce_* (int32 state, exact in fp32 up to 2^24)
 *   WAGG_CELL_SPELL_AMOUNT   the sum over the hot entries of  (double)X[t, j] + offset
 *   WAGG_CELL_SPELL_EXCESS   ... of  ((double)X[t, j] + offset) - (double)thr[k][m][j]   (below = 0), or of
 *                            (double)thr[k][m][j] - ((double)X[t, j] + offset)            (below = 1)
 * The two sums have no run counter: min_length must be 1 (WAGG_EINVAL otherwise).  Each term is two separately rounded fp64
 * operations; the terms are added one at a time IN LIST ORDER to an fp64 accumulator that starts at 0, cast once on the store.
 * The sequential order is the definition: a NumPy loop reproduces the bits (tests/cell_spell_ref.py).
 * Arguments otherwise as for wagg_spell_reduce_*.  Rows are read in 16-byte pieces when X_dev AND thr_dev are 16-byte aligned and
 * ldx, ldt (M > 1) and thr_kstride (n_thr > 1) are multiples of a piece; otherwise element by element, with the same results.
 * work_dev / work_bytes are IGNORED: a list is never split, and the family has no work-size query.  Every bad argument is
 * WAGG_EINVAL with a message, decided before any device call.  Plane k of a many-level call is the plane of the call with level
 * k alone.                                                                                                                       */
#define WAGG_CELL_SPELL_MAX 64
#define WAGG_CELL_SPELL_GROUP 4
#define WAGG_CELL_SPELL_AMOUNT 3
#define WAGG_CELL_SPELL_EXCESS 4
int wagg_cell_spells_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                         const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                         double offset, const float *thr_dev, int n_thr, int64_t ldt, int64_t thr_kstride,
                         const int32_t *plane_of_period_dev, int32_t M, int min_length, int stat, int below, int flags,
                         float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes,
                         void *stream);
int wagg_cell_spells_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                         const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                         double offset, const double *thr_dev, int n_thr, int64_t ldt, int64_t thr_kstride,
                         const int32_t *plane_of_period_dev, int32_t M, int min_length, int stat, int below, int flags,
                         double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev, int64_t work_bytes,
                         void *stream);

/* ---- ... with a threshold plane PER ROW: calendar-day thresholds inside a period (0.17.0) ---------------------------------------
 * wagg_cell_spells_* reads one plane per period.  ETCCDI's TX90p / TN10p / WSDI / CSDI compare each day with the percentile of its
 * own calendar day, so inside an annual period the plane changes from row to row.  wagg_row_cell_spells_* take
 * wagg_cell_spells_*'s arguments with
 *   plane_of_row_dev   a DEVICE int32[T], never NULL, in place of plane_of_period_dev: entry i of period p's list, with row
 *                      t = rows[i] in [0, T), reads plane m = plane_of_row_dev[t] (one scalar per row, as doy_dev[t] is).
 * THE DEFINITION is wagg_cell_spells_*'s text with these changes.  HOT is  X[t, j] >= c  (below: < c)  with  c = ceilT((double)
 * thr[k][m][j] - offset)  formed per row by the same rule; with offset == 0, c is the threshold itself.  Runs, gaps, seasons, NaN
 * days, the truncation at period boundaries and bit 0 of status_dev are unchanged.  A list is never split; work_dev / work_bytes
 * are ignored.  WAGG_CELL_SPELL_EXCESS subtracts the raw threshold OF THAT ROW; amount and excess stay sequential fp64 sums in list
 * order.  NaN THRESHOLDS: out[k][p][j] is NaN if any COUNTED entry of period p had a NaN threshold for cell j and level k -- a
 * counted entry being one whose row lies in the field and on which the cell is in season.  No threshold (and no field value) is
 * loaded for a 16-byte piece none of whose cells is in season; it still ends the runs.  CONSEQUENCE: a cell with no counted entry
 * in a period gives 0, where wagg_cell_spells_* writes NaN for a NaN threshold even then.  PLANE INDICES: without
 * WAGG_PERIOD_ROWS_CHECKED the library's blocking look also checks plane_of_row_dev[rows[i]] in [0, M) for every listed entry whose
 * row lies in the field (WAGG_EINVAL before any launch); with the flag, a block that meets an out-of-range index reads no threshold
 * for that row, writes NaN for its whole period in every plane and sets bit 2 of status_dev.  Rows that no list names need no valid
 * plane.  The kernel reads (1 + n_thr) x the bytes of the listed rows: every counted row reads its own piece of n_thr planes
 * (tests/cell_spell_rows_ref.py is the NumPy twin).  STILL NOT BUILT: the percent-of-days form, ETCCDI's in-base
 * bootstrap; runs that continue across a period boundary are built for the plain thresholds only (wagg_spell_span_*).        */
int wagg_row_cell_spells_f32(const float *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                              const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                              double offset, const float *thr_dev, int n_thr, int64_t ldt, int64_t thr_kstride,
                              const int32_t *plane_of_row_dev, int32_t M, int min_length, int stat, int below, int flags,
                              float *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                              int64_t work_bytes, void *stream);
int wagg_row_cell_spells_f64(const double *X_dev, int64_t T, int64_t n, int64_t ldx, const int32_t *row_begin_dev,
                              const int32_t *rows_dev, int32_t P, int64_t n_rows, const int32_t *doy_dev, const int32_t *win_dev,
                              double offset, const double *thr_dev, int n_thr, int64_t ldt, int64_t thr_kstride,
                              const int32_t *plane_of_row_dev, int32_t M, int min_length, int stat, int below, int flags,
                              double *out_dev, int64_t ldo, int64_t out_pstride, int32_t *status_dev, void *work_dev,
                              int64_t work_bytes, void *stream);

/* ---- packed rows: only the quads a segment table references, as a device matrix (0.9.0) ---------------------------------------
 * A single segment-table plan with a whole-line chunking (wagg_plan_info.lines) knows the distinct aligned 4-cell QUADS of a
 * grid row that hold a referenced cell (c2-real: a third of the row).  Its compact row lays them side by side in grid order:
 * quad i of the sorted distinct referenced quads at positions 4i .. 4i + 3, Gq cells in all -- the row the lines-only host
 * path ships (WAGG_HOST_LINES).  Here that row becomes a (T, Gq) device matrix of its own, for work that sums the field over
 * time first: the row-list reductions above take it with n = Gq (a per-cell vector such as win_dev gathered through
 * wagg_plan_compact_cells), and wagg_apply with WAGG_APPLY_COMPACT_ROWS contracts what they leave.  The map belongs to an
 * element type (elem_bytes 4 / 8: the fp32 and fp64 chunkings differ in the quads they count as referenced).
 *   wagg_plan_compact_info    *Gq = cells of the compact row; 0: the plan has none for that element type (region-shaped
 *                             chunkings only, WAGG_PLAN_NO_LINES and the other kernel-form flags, many-plans)
 *   wagg_plan_compact_cells   cell_of_pos_host[pos] = the grid cell at position pos, Gq values (WAGG_EUNSUPPORTED if Gq = 0)
 *   wagg_pack_rows_*          out[t][pos] = X[t][cell_of_pos[pos]] for device-resident rows (ldx >= G).  With X2_dev (tasmax
 *                             beside tasmin; same ldx) a packed row holds field 0 then field 1: out[t][Gq + pos] = X2[t][..],
 *                             ldo >= 2 * Gq.  One 16-byte piece per lane; bases or pitches that are not 16-byte aligned take
 *                             an element-wise kernel.  Asynchronous on `stream` (the first call of a plan and element type
 *                             uploads the quad table, which blocks once).
 *   wagg_pack_rows_host_*     the same from HOST arrays through the gather of the lines-only host path: host threads pack
 *                             the quads, only they cross PCIe (wagg_host_stats.lines_h2d_bytes), every block is copied into
 *                             its rows of out_dev.  Blocking.  Taken when the packed row is <= 80 % of the row, the field
 *                             >= 64 MiB, at least ten packing threads can be had and the ring is free; otherwise
 *                             WAGG_EUNSUPPORTED with nothing queued: the caller uploads the field and packs on the device.
 *                             flags: 0 or WAGG_HOST_PIN (which has nothing to lock here: X is read by the CPU).           */
int wagg_plan_compact_info(const wagg_plan *plan, int elem_bytes, int64_t *Gq);
int wagg_plan_compact_cells(const wagg_plan *plan, int elem_bytes, int32_t *cell_of_pos_host /* Gq */);
int wagg_pack_rows_f32(const wagg_plan *plan, const float *X_dev, const float *X2_dev /* NULL or tasmax */, int64_t T, int64_t ldx,
                       float *out_dev, int64_t ldo, void *stream);
int wagg_pack_rows_f64(const wagg_plan *plan, const double *X_dev, const double *X2_dev /* NULL or tasmax */, int64_t T, int64_t ldx,
                       double *out_dev, int64_t ldo, void *stream);
int wagg_pack_rows_host_f32(const wagg_plan *plan, const float *X_host, const float *X2_host, int64_t T, int64_t ldx, float *out_dev,
                            int64_t ldo, int flags);
int wagg_pack_rows_host_f64(const wagg_plan *plan, const double *X_host, const double *X2_host, int64_t T, int64_t ldx, double *out_dev,
                            int64_t ldo, int flags);

#ifdef __cplusplus
}
#endif
#endif /* WAGG_H */
