"""ctypes binding of include/dann.h (libdann_hip.so).

The product path has no CPU fallback: if the HIP library is missing or fails to load,
importing this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DANN_LIB_PATH: developer hook for A/B builds of the library (scratch/); the default is the in-tree build
LIB_PATH = os.environ.get("DANN_LIB_PATH") or os.path.join(_HERE, "libdann_hip.so")

F32, F16, U8, I8, SQ8, PQ = 0, 1, 2, 3, 4, 5
SQ1, SQ4 = 17, 20  # packed scalar-quantised rows: 16 + bits
SPH1, SPH2, SPH4 = 33, 34, 36  # spherically quantised rows (RaBitQ): 32 + bits
# dann_query_layout (iface::QueryLayout): the byte image of a spherical index's queries
QUERY_SAME_AS_DATA, QUERY_FOUR_BIT_TRANSPOSED, QUERY_SCALAR_QUANTIZED, QUERY_FULL_PRECISION = 0, 1, 2, 3
QUERY_EIGHT_BIT = 8  # MinMaxQuery::EightBit: set with dann_set_query_dtype(MM8), never with dann_set_query_layout
MM1, MM2, MM4, MM8 = 49, 50, 52, 56  # MinMax-quantised rows: 48 + bits
COSINE, INNER_PRODUCT, L2, COSINE_NORMALIZED = 0, 1, 2, 3
OK, EINVAL, ELENGTH, EBOUNDS, ETOOLONG, EHIP, ENOMEM, EOVERFLOW, EUNSUPPORTED, EINTERNAL, EBUSY = (
    0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10)
IBC_NONE, IBC_ALL = 0, 0xFFFFFFFF
TIE_POSITION, TIE_RUST = 0, 1  # dann_set_prune_tie_order
MAXSIM_KERNEL, MAXSIM_REFERENCE = 0, 1  # the two orders of dann_maxsim_batch / dann_chamfer_rerank_batch
BUILD_MFMA_BACKEDGE, BUILD_MFMA_POOL, BUILD_ROW_KERNEL_ONLY = 1, 2, 4
CONSOLIDATE_COMPLETE, CONSOLIDATE_DELETED = 0, 1  # ConsolidateKind (dann_consolidate out_kind)
CONSOLIDATE_DROP_DELETED = 1  # dann_consolidate flag
DEGREE_SKIP_DELETED = 1  # dann_degree_stats flag
FLAT_SKIP_DELETED = 1  # dann_flat_search_batch flag
INPLACE_VISITED_AND_TOPK, INPLACE_TWO_HOP_AND_ONE_HOP, INPLACE_ONE_HOP = 0, 1, 2  # dann_inplace_delete_params.method
INPLACE_COUNTERS = 9
# dann_transform_parts.kind (TransformKind); RANDOM_ROTATION is reserved (DANN_EUNSUPPORTED)
TRANSFORM_NULL, TRANSFORM_PADDING_HADAMARD, TRANSFORM_DOUBLE_HADAMARD, TRANSFORM_RANDOM_ROTATION = 0, 1, 2, 3


class Config(C.Structure):
    """dann_config == provider::Config + Full::new (diskann-inmem/src/provider.rs:160-217)."""
    _fields_ = [("dtype", C.c_int32), ("metric", C.c_int32), ("dim", C.c_uint32), ("capacity", C.c_uint32),
                ("max_degree", C.c_uint32), ("num_start_points", C.c_uint32), ("row_stride", C.c_uint32),
                ("device", C.c_int32), ("sq_scale", C.c_float), ("sq_shift_norm_sq", C.c_float),
                ("pq_chunks", C.c_uint32), ("inline_tags", C.c_uint32)]


class BuildConfig(C.Structure):
    """dann_build_config == graph::config::Builder (diskann/src/graph/config/mod.rs:261-338)."""
    _fields_ = [("pruned_degree", C.c_uint32), ("max_degree", C.c_uint32), ("l_build", C.c_uint32),
                ("alpha", C.c_float), ("max_occlusion_size", C.c_uint32), ("max_backedges", C.c_uint32),
                ("intra_batch_candidates", C.c_uint32), ("saturate_after_prune", C.c_uint32)]


class Filter(C.Structure):
    """dann_filter == a QueryLabelProvider (diskann/src/graph/ext/labeled.rs:44-68) as a bitmap over slots."""
    _fields_ = [("mode", C.c_uint32), ("bits", C.c_void_p), ("stride_words", C.c_uint64),
                ("adaptive_samples", C.c_uint32), ("adaptive_scale", C.c_double), ("matched_cap", C.c_uint32)]


RNG_INDEX_FN = C.CFUNCTYPE(C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64)
RNG_F64_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_uint32, C.c_double)


class FlatFilter(C.Structure):
    """dann_flat_filter: the bitmaps of an exhaustive scan (host memory; device memory in the _device forms)"""
    _fields_ = [("bits", C.c_void_p), ("stride_words", C.c_uint64)]


class Diverse(C.Structure):
    """dann_diverse: DiverseSearchParams without the attribute provider (dann_set_attributes holds the values)"""
    _fields_ = [("diverse_k", C.c_uint32), ("total_k", C.c_uint32)]


class InplaceDeleteParams(C.Structure):
    """dann_inplace_delete_params: graph::InplaceDeleteMethod + num_to_replace"""
    _fields_ = [("method", C.c_uint32), ("k_value", C.c_uint32), ("l_value", C.c_uint32), ("num_to_replace", C.c_uint32)]


class DegreeStats(C.Structure):
    """dann_degree_summary == DegreeStats (index.rs:2191-2239) + the exact totals behind avg_degree"""
    _fields_ = [("max_degree", C.c_uint32), ("avg_degree", C.c_float), ("min_degree", C.c_uint32), ("reserved", C.c_uint32),
                ("cnt_less_than_two", C.c_uint64), ("points", C.c_uint64), ("total", C.c_uint64)]


NO_ATTRIBUTE = 0xFFFFFFFF  # DANN_NO_ATTRIBUTE: AttributeValueProvider::get returns None


class Rng(C.Structure):
    """dann_rng: the caller's generator for the two random draws of k-means++ (plusplus.rs:417, 440-444)."""
    _fields_ = [("ctx", C.c_void_p), ("uniform_index", RNG_INDEX_FN), ("uniform_f64", RNG_F64_FN)]


COMM_ALL_GATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


class CommOps(C.Structure):
    """dann_comm_ops: a caller-supplied all-gather over device buffers (tests: gloo through host memory)."""
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_uint32), ("world", C.c_uint32), ("all_gather", COMM_ALL_GATHER_FN)]


class ServerConfig(C.Structure):
    """dann_server_config: the resident search server (dann_server_start)."""
    _fields_ = [("l_value", C.c_uint32), ("k", C.c_uint32), ("workers", C.c_uint32), ("ring", C.c_uint32),
                ("idle_timeout_us", C.c_uint32)]


class TransformParts(C.Structure):
    """dann_transform_parts: the arguments of Transform::try_from_parts (host pointers, copied by dann_transform_create)."""
    _fields_ = [("kind", C.c_int32), ("dim", C.c_uint32), ("signs0", C.c_void_p), ("signs0_len", C.c_uint32),
                ("signs1", C.c_void_p), ("signs1_len", C.c_uint32), ("padded_dim", C.c_uint32),
                ("subsample", C.c_void_p), ("subsample_len", C.c_uint32)]


class SphericalParts(C.Structure):
    """dann_spherical_parts: metric, shift (host pointer, copied by dann_spherical_create) and pre_scale of a
    SphericalQuantizer."""
    _fields_ = [("metric", C.c_int32), ("shift", C.c_void_p), ("pre_scale", C.c_float)]


class SearchStats(C.Structure):
    _fields_ = [("cmps", C.c_uint32), ("hops", C.c_uint32), ("result_count", C.c_uint32), ("status", C.c_uint32),
                ("written", C.c_uint32)]


# every symbol include/dann.h declares: name -> (restype, argtypes)
_vp, _u32, _i32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64, C.c_float
_P = C.POINTER
SYMBOLS = {
    "dann_layer_bytes": (_i32, [_i32, _u32]),
    "dann_inmem2_row_stride": (_i32, [_i32, _u32]),
    "dann_index_create": (_i32, [_P(Config), _vp, _u64, _P(_vp)]),
    "dann_index_destroy": (_i32, [_vp]),
    "dann_index_max_degree": (_i32, [_vp]),
    "dann_index_get_config": (_i32, [_vp, _P(Config)]),
    "dann_set_element": (_i32, [_vp, _u32, _vp, _u64]),
    "dann_set_elements": (_i32, [_vp, _u32, _u32, _vp, _u64]),
    "dann_get_element": (_i32, [_vp, _u32, _vp, _u64]),
    "dann_set_elements_device": (_i32, [_vp, _u32, _u32, _vp, _u64]),
    "dann_index_device_pointers": (_i32, [_vp, _P(_vp), _P(_vp)]),
    "dann_search_record_queries": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _vp]),
    "dann_upload_store": (_i32, [_vp, _vp, _u64, _u32]),
    "dann_set_tags": (_i32, [_vp, _u32, _u32, _vp]),
    "dann_get_tags": (_i32, [_vp, _u32, _u32, _vp]),
    "dann_set_external_ids": (_i32, [_vp, _u32, _u32, _vp]),
    "dann_to_external": (_i32, [_vp, _vp, _u64, _vp]),
    "dann_get_neighbors": (_i32, [_vp, _u32, _vp, _u32, _P(_u32)]),
    "dann_set_neighbors": (_i32, [_vp, _u32, _vp, _u32]),
    "dann_append_neighbors": (_i32, [_vp, _u32, _vp, _u32]),
    "dann_set_neighbors_bulk": (_i32, [_vp, _vp, _u32, _vp]),
    "dann_upload_graph": (_i32, [_vp, _vp, _u64]),
    "dann_download_graph": (_i32, [_vp, _vp, _u64]),
    "dann_distance": (_i32, [_vp, _vp, _u64, _vp, _u64, _P(_f32)]),
    "dann_distance_pairs": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "dann_query_create": (_i32, [_vp, _vp, _u64, _P(_vp)]),
    "dann_query_destroy": (_i32, [_vp]),
    "dann_query_distance": (_i32, [_vp, _vp, _u64, _P(_f32)]),
    "dann_expand_beam": (_i32, [_vp, _vp, _u32, _vp, _vp, _P(_u32)]),
    "dann_expand_beam_batch": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "dann_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "dann_search_batch_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "dann_range_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _f32, _i32, _f32, _f32, _f32, _u32, _u32, _vp, _vp,
                                       _vp, _vp]),
    "dann_filtered_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _P(Filter), _vp, _vp, _vp]),
    "dann_filtered_range_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _f32, _i32, _f32, _f32, _f32, _u32, _u32,
                                                _P(Filter), _vp, _vp, _vp, _vp]),
    "dann_paged_begin": (_i32, [_vp, _vp, _u32, _u32, _u32, _P(_vp)]),
    "dann_paged_next": (_i32, [_vp, _u32, _vp, _vp, _vp]),
    "dann_paged_end": (_i32, [_vp]),
    "dann_rerank_batch": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp]),
    "dann_rerank_batch_device": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp]),
    "dann_flat_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "dann_flat_search_batch_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "dann_flat_filtered_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _P(FlatFilter), _vp, _vp, _vp]),
    "dann_flat_range_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _f32, _i32, _f32, _u32, _P(FlatFilter), _u32, _vp,
                                            _vp, _vp, _vp]),
    "dann_flat_filtered_search_batch_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _P(FlatFilter), _vp, _vp,
                                                      _vp]),
    "dann_flat_range_search_batch_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _f32, _i32, _f32, _u32, _P(FlatFilter), _u32,
                                                   _vp, _vp, _vp, _vp]),
    "dann_pq_linear_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _P(FlatFilter), _vp, _vp, _vp]),
    "dann_pq_linear_search_batch_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _P(FlatFilter), _vp, _vp, _vp]),
    "dann_search_record_batch": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _vp]),
    "dann_mvset_create": (_i32, [_i32, _i32, _u32, _u32, _vp, _vp, _P(_vp)]),
    "dann_mvset_destroy": (_i32, [_vp]),
    "dann_mvset_info": (_i32, [_vp, _P(_i32), _P(_u32), _P(_u32), _P(_u64)]),
    "dann_mvset_set_query_dtype": (_i32, [_vp, _i32]),
    "dann_mvset_get_query_dtype": (_i32, [_vp, _P(_i32)]),
    "dann_maxsim_batch": (_i32, [_vp, _i32, _vp, _vp, _u32, _vp, _u32, _vp, _vp]),
    "dann_maxsim_batch_device": (_i32, [_vp, _i32, _vp, _vp, _u32, _vp, _u32, _vp, _vp]),
    "dann_chamfer_rerank_batch": (_i32, [_vp, _i32, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp]),
    "dann_chamfer_rerank_batch_device": (_i32, [_vp, _i32, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp]),
    "dann_prune_batch": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _vp, _vp, _vp, _i32, _vp]),
    "dann_insert_batch": (_i32, [_vp, _P(BuildConfig), _vp, _u32]),
    "dann_insert": (_i32, [_vp, _P(BuildConfig), _u32]),
    "dann_insert_batch_candidates": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _u32, _u32, _vp]),
    "dann_insert_batch_commit": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _vp]),
    "dann_insert_batch_commit_part": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _vp, _u32, _u32, _vp, _u32, _P(_u32)]),
    "dann_apply_neighbor_rows_device": (_i32, [_vp, _vp, _u32]),
    "dann_build": (_i32, [_vp, _P(BuildConfig), _u32, _u32, _f32, _u32]),
    "dann_set_build_options": (_i32, [_vp, _u32]),
    "dann_build_counters": (_i32, [_vp, _vp, _u32]),
    "dann_delete_points": (_i32, [_vp, _vp, _u32]),
    "dann_get_deleted": (_i32, [_vp, _u32, _u32, _vp]),
    "dann_set_attributes": (_i32, [_vp, _u32, _u32, _vp]),
    "dann_get_attributes": (_i32, [_vp, _u32, _u32, _vp]),
    "dann_diverse_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _P(Diverse), _vp, _vp, _vp]),
    "dann_consolidate": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _u32, _vp, _vp]),
    "dann_inplace_delete": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _P(InplaceDeleteParams), _vp]),
    "dann_drop_deleted_neighbors": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _u32, _vp]),
    "dann_prune_range": (_i32, [_vp, _P(BuildConfig), _vp, _u32, _u32, _vp]),
    "dann_count_reachable": (_i32, [_vp, _vp, _u32, _P(_u64), _P(_u32), _vp]),
    "dann_degree_stats": (_i32, [_vp, _vp, _u32, _u32, _P(DegreeStats)]),
    "dann_debug_gram_tiles": (_i32, [_i32, _i32, _vp, _u32, _u32, _u32, _vp, _vp]),
    "dann_save_graph": (_i32, [_vp, C.c_char_p]),
    "dann_load_graph": (_i32, [_vp, C.c_char_p, _P(_u32), _P(_u64), _P(_u64)]),
    "dann_save_vectors_bin": (_i32, [_vp, C.c_char_p, _u32, _u32]),
    "dann_load_vectors_bin": (_i32, [_vp, C.c_char_p, _u32, _P(_u32)]),
    "dann_set_pq_table": (_i32, [_vp, _vp, _vp]),
    "dann_pq_pack_neighbors": (_i32, [_vp]),
    "dann_set_query_layout": (_i32, [_vp, _i32]),
    "dann_get_query_layout": (_i32, [_vp]),
    "dann_query_bytes": (_i32, [_vp]),
    "dann_set_query_dtype": (_i32, [_vp, _i32]),
    "dann_get_query_dtype": (_i32, [_vp, _P(_i32)]),
    "dann_sq8_train": (_i32, [_i32, _vp, _u64, _u32, C.c_double, _vp, _vp, _vp]),
    "dann_sq8_compress": (_i32, [_i32, _vp, _u32, _u32, _vp, _f32, _vp]),
    "dann_sq_compress": (_i32, [_i32, _i32, _vp, _u32, _u32, _vp, _f32, _vp]),
    "dann_minmax_compress": (_i32, [_i32, _i32, _vp, _u32, _u32, _f32, _vp, _vp]),
    "dann_medoid": (_i32, [_i32, _i32, _vp, _u64, _u32, _u64, _P(C.c_int64), _vp, _vp]),
    "dann_medoid_device": (_i32, [_i32, _i32, _vp, _u64, _u32, _u64, _P(C.c_int64), _vp, _vp]),
    "dann_transform_create": (_i32, [_i32, _P(TransformParts), _P(_vp)]),
    "dann_transform_destroy": (_i32, [_vp]),
    "dann_transform_input_dim": (_i32, [_vp]),
    "dann_transform_output_dim": (_i32, [_vp]),
    "dann_transform_apply": (_i32, [_vp, _vp, _u32, _vp]),
    "dann_transform_apply_device": (_i32, [_vp, _vp, _u64, _u32, _vp, _u64]),
    "dann_minmax_quantize": (_i32, [_vp, _i32, _f32, _vp, _u32, _vp, _vp]),
    "dann_minmax_quantize_device": (_i32, [_vp, _i32, _f32, _vp, _u64, _u32, _vp, _u64, _vp]),
    "dann_spherical_create": (_i32, [_vp, _P(SphericalParts), _P(_vp)]),
    "dann_spherical_destroy": (_i32, [_vp]),
    "dann_spherical_shift_norm_sq": (_i32, [_vp, _P(_f32)]),
    "dann_spherical_compress": (_i32, [_vp, _i32, _vp, _u32, _vp]),
    "dann_spherical_compress_device": (_i32, [_vp, _i32, _vp, _u64, _u32, _vp, _u64]),
    "dann_spherical_compress_queries": (_i32, [_vp, _i32, _i32, _vp, _u32, _vp]),
    "dann_spherical_compress_queries_device": (_i32, [_vp, _i32, _i32, _vp, _u64, _u32, _vp, _u64]),
    "dann_pq_build_lut": (_i32, [_i32, _i32, _vp, _vp, _u32, _u32, _vp, _u32, _vp]),
    "dann_pq_compress": (_i32, [_i32, _vp, _u32, _vp, _u32, _u32, _vp, _u64, _vp]),
    "dann_pq_lloyds": (_i32, [_i32, _vp, _u64, _u32, _vp, _u32, _u32, _vp, _u32, _vp, _vp]),
    "dann_pq_scan": (_i32, [_i32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "dann_pq_kmeanspp": (_i32, [_i32, _vp, _u64, _u32, _vp, _u32, _u32, _P(Rng), _vp, _vp]),
    "dann_pq_train": (_i32, [_i32, _vp, _u64, _u32, _vp, _u32, _u32, _u32, _P(Rng), _vp]),
    "dann_abi_version": (_i32, []),
    "dann_debug_stream_read_gbps": (_i32, [_i32, _u64, _u32, _P(C.c_double)]),
    "dann_last_error": (_i32, [C.c_char_p, _u64]),
    "dann_kernel_time": (_i32, [_vp, _i32, _P(C.c_double), _P(_u64)]),
    "dann_kernel_time_reset": (_i32, [_vp]),
    "dann_set_visited_bits": (_i32, [_vp, _u32]),
    "dann_set_visited_format": (_i32, [_vp, _u32]),
    "dann_set_max_concurrency": (_i32, [_vp, _u32]),
    "dann_set_prune_tie_order": (_i32, [_vp, _u32]),
    "dann_comm_create_callbacks": (_i32, [_vp, _P(_vp)]),
    "dann_comm_rccl_unique_id": (_i32, [_vp]),
    "dann_comm_create_rccl": (_i32, [_vp, _u32, _u32, _i32, _P(_vp)]),
    "dann_comm_create_local": (_i32, [_vp, _u32, _vp]),
    "dann_comm_destroy": (_i32, [_vp]),
    "dann_comm_rank": (_i32, [_vp]),
    "dann_comm_world": (_i32, [_vp]),
    "dann_comm_all_gather_device": (_i32, [_vp, _i32, _vp, _vp, _u64]),
    "dann_build_sharded": (_i32, [_vp, _vp, _P(BuildConfig), _u32, _u32, _f32, _u32, _vp]),
    "dann_search_sharded": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "dann_memcpy_device": (_i32, [_i32, _vp, _vp, _u64, _i32]),
    "dann_multi_create": (_i32, [_P(Config), _vp, _u64, _vp, _u32, _P(_vp)]),
    "dann_multi_destroy": (_i32, [_vp]),
    "dann_multi_size": (_i32, [_vp]),
    "dann_multi_replica": (_vp, [_vp, _u32]),
    "dann_multi_set_elements": (_i32, [_vp, _u32, _u32, _vp, _u64]),
    "dann_multi_build": (_i32, [_vp, _P(BuildConfig), _u32, _u32, _f32, _u32, _vp]),
    "dann_multi_search_batch": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "dann_server_start": (_i32, [_vp, _vp]),
    "dann_server_stop": (_i32, [_vp]),
    "dann_search_submit": (_i32, [_vp, _vp, _P(_u64)]),
    "dann_search_poll": (_i32, [_vp, _u64]),
    "dann_search_wait": (_i32, [_vp, _u64, _vp, _vp, _vp]),
    "dann_server_stats": (_i32, [_vp, _P(_u64), _P(_u64)]),
    "dann_debug_concurrent_callers": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp,
                                             _P(C.c_double)]),
    "dann_debug_set": (_i32, [_vp, _i32, C.c_double]),
    "dann_debug_get": (_i32, [_vp, _i32, _P(C.c_double)]),
    "dann_debug_search_families": (_i32, [_vp, _P(_u64), _P(C.c_double)]),
    "dann_debug_small_call_stats": (_i32, [_vp, _P(_u64)]),
    "dann_debug_sched_pivots": (_i32, [_vp, _vp, _u32, _P(_u32), _P(_u32), _P(_f32)]),
    "dann_debug_family_name": (C.c_char_p, [_i32]),
    "dann_debug_pq_rolling_sum_stats": (_i32, [_i32, _P(_u64), _i32]),
    "dann_debug_medoid_times": (_i32, [_i32, _i32, _vp, _u64, _u32, _u64, _P(C.c_int64), _vp, _P(C.c_double)]),
    "dann_debug_mvset_kernel_time": (_i32, [_vp, _i32, _P(C.c_double), _P(_u64)]),
}

# dann_debug.h: development switches (dann_debug_set) and kernel families (dann_debug_search_families)
DBG_KEYS = {"tune_off": 0, "tune_on": 1, "pair_min_queries": 2, "team_max_queries": 3, "host_pipeline": 4,
            "sweep_one_by_one": 5, "pool_gram": 6, "gram_cols": 7, "gram_escale": 8, "backedge_gram_rows": 9,
            "server_max_resident_us": 10, "verbose": 11, "ht16_open_eighths": 12, "backedge_single_pool": 13,
            "ht16_max_probes": 14, "host_chunk": 15, "gram_f16_widen": 16, "time_small_launches": 17,
            "sched_min_queries": 18, "diverse_pool": 19, "sched_lloyd_iters": 20, "flat_chunk_rows": 21}
DBG_FLAT_CHUNK_ROWS = DBG_KEYS["flat_chunk_rows"]
FAMILIES = ("one_wave", "team", "pair", "persistent", "server", "pq_lut", "diverse")

_lib = None


def lib():
    """Load libdann_hip.so (raises if it is absent: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m diskann_amd.build` "
                "(or __graft_entry__.build()).  diskann_amd has no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own libamdhip64; two HIP runtimes in one process cannot
        # both own the GPU ("No HIP GPUs are available" for whichever initialises second).  If torch
        # is installed, load it first so that libdann_hip.so binds to the runtime torch uses.
        try:
            import torch  # noqa: F401
        except Exception:  # torch is optional for the library itself
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


class DannError(RuntimeError):
    """ANNError analogue: carries the DANN_E* status and the library's message."""

    def __init__(self, status, where):
        buf = C.create_string_buffer(512)
        lib().dann_last_error(buf, 512)
        self.status = status
        super().__init__(f"{where} failed with status {status}: {buf.value.decode(errors='replace')}")


def check(status, where):
    if status < 0:
        raise DannError(status, where)
    return status
