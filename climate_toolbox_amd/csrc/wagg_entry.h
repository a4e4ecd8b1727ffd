// The typed apply layer (namespace wagg::entry): one function template per apply, on the element type T (float or double).
// It is what wagg_apply() (wagg_desc.hip) dispatches a descriptor to -- run_segment<T> / run_dense<T> call entry::x<T> -- and
// what code INSIDE the library calls when it needs an apply (the host pipelines launch entry::apply<T> per block, the shard
// group per shard).  Each template is defined in the translation unit of its plan kind (wagg_sparse.hip, wagg_dense.hip,
// wagg_shard.hip) and instantiated there for float and double; the `dense_` prefix marks the dense-family plan kind.
// The exported wagg_*apply*_f32/_f64 symbols of include/wagg.h are wrappers in wagg_desc.hip that fill a wagg_apply_desc and
// call wagg_apply(); argument meaning: wagg.h.
#pragma once
#include "../../include/wagg.h"

namespace wagg {
namespace entry {
template <typename T> int apply(const wagg_plan *plan, const T *X_dev, int64_t Tn, int64_t ldx, int layout, T *out_dev, int64_t ldo, int out_layout, void *stream);
// WAGG_APPLY_COMPACT_ROWS: X_dev holds packed rows (wagg_pack.hip), ldx >= Gq
template <typename T> int apply_compact(const wagg_plan *plan, const T *X_dev, int64_t Tn, int64_t ldx, T *out_dev, int64_t ldo, void *stream);
template <typename T> int apply_host_ex(const wagg_plan *plan, const T *X_host, int64_t Tn, int64_t ldx, int layout, T *out_host, int64_t ldo, int out_layout, int flags);
template <typename T> int apply_host_multi(const wagg_plan *const *plans, const int *devices, int n_devices, const T *X_host, int64_t Tn, int64_t ldx, T *out_host, int64_t ldo, int flags);
template <typename T> int apply_poly(const wagg_plan *plan, const T *X_dev, int64_t Tn, int64_t ldx, int layout, double offset, int pow_first, int n_pow, T *out_dev, int64_t ldo, int64_t out_pstride, int out_layout, void *stream);
template <typename T> int apply_poly_host(const wagg_plan *plan, const T *X_host, int64_t Tn, int64_t ldx, double offset, int pow_first, int n_pow, T *out_host, int64_t ldo, int64_t out_pstride, int flags);
template <typename T> int apply_edd(const wagg_plan *plan, const T *tasmin_dev, const T *tasmax_dev, int64_t Tn, int64_t ldx, int layout, double offset, const double *thresholds, int n_thr, T *out_dev, int64_t ldo, int64_t out_pstride, int out_layout, void *stream);
template <typename T> int apply_edd_host(const wagg_plan *plan, const T *tasmin_host, const T *tasmax_host, int64_t Tn, int64_t ldx, double offset, const double *thresholds, int n_thr, T *out_host, int64_t ldo, int64_t out_pstride, int flags);
template <typename T> int apply_sharded(wagg_shard_group *g, const wagg_plan *const *plans, const T *const *X_dev, const int64_t *rows, int64_t ldx, T *out_root, int64_t ldo, int root);
// (dense applies: exact = WAGG_APPLY_EXACT_F32, the fp32-pipe kernel instead of the split form; fp64 plans ignore it)
template <typename T> int dense_apply(wagg_dense *d, const T *X_dev, int64_t Tn, int64_t ldx, T *out_dev, int64_t ldo, int ksplit, void *stream, bool exact = false);
template <typename T> int dense_apply_poly(wagg_dense *d, const T *X_dev, int64_t Tn, int64_t ldx, double offset, int power, T *out_dev, int64_t ldo, int ksplit, void *stream, bool exact = false);
template <typename T> int dense_apply_edd(wagg_dense *d, const T *tasmin_dev, const T *tasmax_dev, int64_t Tn, int64_t ldx, double offset, double threshold, T *out_dev, int64_t ldo, int ksplit, void *stream, bool exact = false);
template <typename T> int dense_apply_host(wagg_dense *d, const T *X_host, int64_t Tn, int64_t ldx, T *out_host, int64_t ldo, int flags, bool exact = false);
template <typename T> int dense_apply_host_multi(wagg_dense *const *plans, const int *devices, int n_devices, const T *X_host, int64_t Tn, int64_t ldx, T *out_host, int64_t ldo, int flags);
template <typename T> int dense_apply_sharded(wagg_shard_group *g, wagg_dense *const *plans, const T *const *X_dev, const int64_t *rows, int64_t ldx, T *out_root, int64_t ldo, int root);
// many-plans (wagg_plan_create_many): the concatenated result of every (level, weighting) plane, from one pass over X
template <typename T> int apply_many(const wagg_plan *plan, const T *X_dev, int64_t Tn, int64_t ldx, int layout, T *out_dev, int64_t ldo, int out_layout, void *stream);
template <typename T> int apply_many_host(const wagg_plan *plan, const T *X_host, int64_t Tn, int64_t ldx, int layout, T *out_host, int64_t ldo, int out_layout, int flags);
bool is_many_plan(const wagg_plan *plan);
}  // namespace entry
}  // namespace wagg
