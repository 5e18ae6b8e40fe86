"""diskann_amd: MI355X-native batched distance / beam-search / RobustPrune path behind the
surface of the reference's diskann-inmem provider (include/dann.h)."""
from ._ffi import (F32, F16, U8, I8, SQ8, SQ1, SQ4, SPH1, SPH2, SPH4, MM1, MM2, MM4, MM8, QUERY_EIGHT_BIT, QUERY_SAME_AS_DATA, QUERY_FOUR_BIT_TRANSPOSED, QUERY_SCALAR_QUANTIZED,
                   QUERY_FULL_PRECISION, PQ, COSINE, INNER_PRODUCT, L2, COSINE_NORMALIZED, IBC_ALL, IBC_NONE, TIE_POSITION, TIE_RUST, MAXSIM_KERNEL, MAXSIM_REFERENCE, BUILD_MFMA_BACKEDGE, BUILD_MFMA_POOL, BUILD_ROW_KERNEL_ONLY, BuildConfig,
                   CONSOLIDATE_COMPLETE, CONSOLIDATE_DELETED, CONSOLIDATE_DROP_DELETED, DEGREE_SKIP_DELETED, DegreeStats, NO_ATTRIBUTE, FLAT_SKIP_DELETED, DBG_FLAT_CHUNK_ROWS,
                   INPLACE_VISITED_AND_TOPK, INPLACE_TWO_HOP_AND_ONE_HOP, INPLACE_ONE_HOP, INPLACE_COUNTERS,
                   Config, DannError, SearchStats, lib)
from .provider import FILTER_INLINE, FILTER_MULTIHOP, Knn, Provider, build_config, NP_DTYPE, STATS_DTYPE, sq8_compress, sq_compress, minmax_compress, medoid, minmax_quantize, minmax_quantize_device, Transform, SphericalCompressor, sq8_train, pq_build_lut, pq_scan, pq_compress, pq_lloyds, pq_kmeanspp, pq_train, pq_rolling_sum_stats

from .sharding import Comm, MultiProvider
from .multivector import MultiVectorSet

__all__ = ["Comm", "MultiProvider", "MultiVectorSet", "MAXSIM_KERNEL", "MAXSIM_REFERENCE", "F32", "F16", "U8", "I8", "SQ8", "SQ1", "SQ4", "SPH1", "SPH2", "SPH4", "MM1", "MM2", "MM4", "MM8", "QUERY_EIGHT_BIT", "minmax_compress", "minmax_quantize", "minmax_quantize_device", "Transform", "SphericalCompressor", "QUERY_SAME_AS_DATA", "QUERY_FOUR_BIT_TRANSPOSED",
           "QUERY_SCALAR_QUANTIZED", "QUERY_FULL_PRECISION", "PQ", "sq8_compress", "sq_compress", "sq8_train", "pq_build_lut", "pq_scan", "pq_compress", "pq_lloyds", "pq_kmeanspp", "pq_train", "pq_rolling_sum_stats", "COSINE", "INNER_PRODUCT", "L2", "COSINE_NORMALIZED", "IBC_ALL", "IBC_NONE", "TIE_POSITION", "TIE_RUST", "BUILD_MFMA_BACKEDGE", "BUILD_MFMA_POOL", "BUILD_ROW_KERNEL_ONLY",
           "CONSOLIDATE_COMPLETE", "CONSOLIDATE_DELETED", "CONSOLIDATE_DROP_DELETED", "DEGREE_SKIP_DELETED", "DegreeStats", "medoid", "NO_ATTRIBUTE", "FLAT_SKIP_DELETED", "DBG_FLAT_CHUNK_ROWS",
           "INPLACE_VISITED_AND_TOPK", "INPLACE_TWO_HOP_AND_ONE_HOP", "INPLACE_ONE_HOP", "INPLACE_COUNTERS",
           "BuildConfig", "Config", "DannError", "SearchStats", "lib", "Knn", "Provider", "build_config", "NP_DTYPE",
           "STATS_DTYPE", "FILTER_INLINE", "FILTER_MULTIHOP"]
