"""ctypes loader for libgranne_hip.so (the C ABI declared in include/granne_hip.h).

There is no fallback: if the library is missing or the GPU is absent, calls raise."""
import ctypes as C
import os

from . import build as _build

F32, I8, F16 = 0, 1, 2  # GRANNE_HIP_F32 / _I8 / _F16 (rows of halves, normalised on read: "angular_f16")
UNUSED = 0xFFFFFFFF
BUILD_ALL = 0xFFFFFFFFFFFFFFFF  # GRANNE_HIP_BUILD_ALL: Builder::build()

OK = 0
ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_OVERFLOW, ERR_IO = -1, -2, -3, -4, -5

OPT_VISITED_SLOTS, OPT_FORCE_SLOW, OPT_SLOW_SLOTS, OPT_SLOW_BLOCKS, OPT_OVERFLOW_SLOTS = 1, 2, 3, 4, 5
OPT_VISITED16, OPT_VISITED16_LG, OPT_LAST_WALKER, OPT_SEARCH_DEPTH, OPT_INLINE_TAILS, OPT_SEEN_MIN = 6, 7, 8, 9, 10, 11
OPT_SKETCH = 12
# concurrent host-pointer calls share launches (granne_amd/csrc/combiner.h); the last two are read-only counters
OPT_COALESCE, OPT_COALESCE_MAX, OPT_COALESCE_WAIT_US, OPT_COALESCED_LAUNCHES, OPT_COALESCED_QUERIES = 13, 14, 15, 16, 17
OPT_LAST_COMPACT_ROWS = 18  # read-only: the last launch ran the compacted row stage of the sketched walkers
OPT_LAST_SPLIT_TAIL = 19  # read-only: the last launch ran its tail blocks as a kernel of their own, behind the walkers'
OPT_LAST_SCAN = 20  # read-only: what the last exact scan ran, one packed word (last_scan() takes it apart)
OPT_FORCE_GENERAL = 21  # 1: no register walker (tests and measurement: the unfiltered baseline of filtered search)
# GRANNE_HIP_SCAN_*: the exact scan's kernel forms, one per rule of its dispatch
(SCAN_NONE, SCAN_RING, SCAN_I8, SCAN_I8_CHUNKED, SCAN_B16_7_4, SCAN_B16_13_2, SCAN_B16_16_1, SCAN_B16_CHUNKED, SCAN_F32_52_4,
 SCAN_F32_100_2, SCAN_F32_128_1) = range(11)
EXACT_TOPK_KMAX = 1024  # GRANNE_HIP_EXACT_TOPK_KMAX
EXACT_TOPK_CAP = 4096  # GRANNE_HIP_EXACT_TOPK_CAP: candidates ranked per query
PF_MAX_STAGES = 8  # GRANNE_HIP_PF_MAX_STAGES: post-filtered search (Granne.search_postfiltered_batch)
PF_FALLBACK_SHORT, PF_FALLBACK_EXACT = 0, 1  # GRANNE_HIP_PF_FALLBACK_*
PF_STAGE_EXACT, PF_STAGE_SHORT = 0xFFFFFFFF, 0xFFFFFFFE  # GRANNE_HIP_PF_STAGE_*: out_stage of a query no stage finished
RANGE_CAP_MAX = 1024  # GRANNE_HIP_RANGE_CAP_MAX: range search (Granne.exact_range, Granne.search_range_batch)
RG_MAX_STAGES = 8  # GRANNE_HIP_RG_MAX_STAGES
RG_FALLBACK_SHORT, RG_FALLBACK_EXACT = 0, 1  # GRANNE_HIP_RG_FALLBACK_*
RG_STAGE_EXACT, RG_STAGE_SHORT = 0xFFFFFFFF, 0xFFFFFFFE  # GRANNE_HIP_RG_STAGE_*: out_stage of a query no stage finished
COALESCE_CALL_MAX = 64  # GRANNE_HIP_COALESCE_CALL_MAX
COALESCE_MAX = 1024  # GRANNE_HIP_COALESCE_MAX
WALKER_NONE, WALKER_REGISTER, WALKER_REGISTER_WIDE, WALKER_GENERAL, WALKER_EXACT = 0, 1, 2, 3, 4
SEARCH_DEPTH = 3  # GRANNE_HIP_SEARCH_DEPTH (the default of OPT_SEARCH_DEPTH)
SEARCH_DEPTH_MAX = 16  # GRANNE_HIP_SEARCH_DEPTH_MAX
SHARDED_OPT_DEPTH, SHARDED_OPT_EXCHANGE = 1, 2
SHARDED_EXCHANGE_PEER, SHARDED_EXCHANGE_RCCL = 0, 1
RW_OPT_SMALL_OPS, RW_OPT_SMALL_LAUNCHES, RW_OPT_SORTED_LAUNCHES = 1, 2, 3  # GRANNE_HIP_RW_OPT_*
RW_OPT_REMOVED, RW_OPT_FILTERED_SEARCHES = 4, 5  # read-only: removed elements; search calls that ran under the tombstones
RW_SMALL_OPS = 2048  # GRANNE_HIP_RW_SMALL_OPS
CODEC_STAGING_DEFAULT = 64 << 20  # GRANNE_HIP_CODEC_STAGING_DEFAULT: the device codec's pinned ring (staging_bytes=0)
CODEC_STAGING_MIN = 64 << 10  # GRANNE_HIP_CODEC_STAGING_MIN: smaller values are raised to it
SE_MATERIALIZED, SE_COMPACT = 0, 1  # GRANNE_HIP_SE_*: the two forms of an index over a SumEmbeddings container


def last_scan(word):
    """GRANNE_HIP_OPT_LAST_SCAN's word (include/granne_hip.h) as a dict: form (SCAN_*), ranges (G), primed (bool),
    prime_ranges (Gs, 0 with fewer than 32 ranges), kk."""
    word = int(word)
    return {"form": word & 0xFF, "ranges": word >> 8 & 0xFFFF, "primed": bool(word >> 24 & 1),
            "prime_ranges": word >> 32 & 0xFF, "kk": word >> 40 & 0xFF}


class GranneHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("granne_hip error %d: %s" % (code, message))
        self.code = code


class BuildConfig(C.Structure):
    """granne_hip_build_config (include/granne_hip.h) = BuildConfig (src/index/mod.rs:198-231)."""
    _fields_ = [
        ("layer_multiplier", C.c_float),
        ("expected_num_elements", C.c_uint64),
        ("num_neighbors", C.c_uint32),
        ("max_search", C.c_uint32),
        ("reinsert_elements", C.c_int),
        ("show_progress", C.c_int),
        ("batch_max", C.c_uint32),
        ("batch_div", C.c_uint32),
    ]


_lib = None

vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int

# name -> (restype, argtypes): every symbol include/granne_hip.h declares
SIGNATURES = {
    "granne_hip_last_error": (C.c_char_p, []),
    "granne_hip_abi_version": (i32, []),
    "granne_hip_device_count": (i32, [C.POINTER(i32)]),
    "granne_hip_index_create": (i32, [C.POINTER(vp), vp, u64, u32, i32, u32, vp, vp, vp, i32]),
    "granne_hip_index_create_csr": (i32, [C.POINTER(vp), vp, u64, u32, i32, u32, vp, vp, vp, i32]),
    "granne_hip_index_create_device": (i32, [C.POINTER(vp), vp, u64, u32, i32, u32, vp, vp, vp, i32, vp]),
    "granne_hip_index_destroy": (None, [vp]),
    "granne_hip_index_len": (u64, [vp]),
    "granne_hip_index_num_elements": (u64, [vp]),
    "granne_hip_index_num_layers": (u32, [vp]),
    "granne_hip_index_layer_len": (u64, [vp, u32]),
    "granne_hip_index_dim": (u32, [vp]),
    "granne_hip_index_dtype": (i32, [vp]),
    "granne_hip_index_device": (i32, [vp]),
    "granne_hip_index_hbm_bytes": (u64, [vp]),
    "granne_hip_index_get_neighbors": (i32, [vp, u64, u32, vp, u32, C.POINTER(u32)]),
    "granne_hip_index_get_element": (i32, [vp, u64, vp]),
    "granne_hip_index_get_sketch": (i32, [vp, u64, u64, vp]),
    "granne_hip_search_batch": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp]),
    "granne_hip_search_batch_device": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search_batches_device": (i32, [vp, u32, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search_begin_device": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, C.POINTER(u64)]),
    "granne_hip_search_end_device": (i32, [vp, u64, vp]),
    "granne_hip_device_malloc": (i32, [C.POINTER(vp), u64, i32]),
    "granne_hip_device_free": (i32, [vp, i32]),
    "granne_hip_copy_to_device": (i32, [vp, vp, u64, i32, vp]),
    "granne_hip_copy_to_host": (i32, [vp, vp, u64, i32, vp]),
    "granne_hip_stream_create": (i32, [C.POINTER(vp), i32]),
    "granne_hip_stream_destroy": (i32, [vp, i32]),
    "granne_hip_stream_synchronize": (i32, [vp, i32]),
    "granne_hip_event_create": (i32, [vp]),
    "granne_hip_event_destroy": (None, [vp]),
    "granne_hip_event_elapsed_ms": (i32, [vp, vp, vp]),
    "granne_hip_search_batch_device_timed": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search": (i32, [vp, vp, u32, u32, vp, vp, C.POINTER(u32)]),
    "granne_hip_normalize_f32_device": (i32, [vp, u64, u32, i32, vp]),
    "granne_hip_quantize_f32_device": (i32, [vp, vp, u64, u32, i32, vp]),
    "granne_hip_f32_to_f16_device": (i32, [vp, vp, u64, u32, i32, vp]),
    "granne_hip_f16_to_f32_device": (i32, [vp, vp, u64, u32, i32, i32, vp]),
    "granne_hip_dist_pairs_device": (i32, [vp, vp, vp, vp, u64, vp, vp]),
    "granne_hip_dists_device": (i32, [vp, vp, u32, vp, u32, vp, vp, vp]),
    "granne_hip_refine_device": (i32, [vp, vp, u32, vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_search_refined_batch_device": (i32, [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search_refined_batch": (i32, [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_index_reorder": (i32, [vp, vp]),
    "granne_hip_index_reorder_by_keys": (i32, [vp, vp, vp]),
    "granne_hip_normalize_f32": (i32, [vp, u64, u32, i32]),
    "granne_hip_quantize_f32": (i32, [vp, vp, u64, u32, i32]),
    "granne_hip_dist_pairs": (i32, [vp, vp, u32, vp, vp, u64, vp]),
    "granne_hip_f32_to_f16": (i32, [vp, vp, u64, u32, i32]),
    "granne_hip_f16_to_f32": (i32, [vp, vp, u64, u32, i32, i32]),
    "granne_hip_synth_rows_device": (i32, [vp, u64, u64, u64, u32, i32, vp]),
    "granne_hip_index_load": (i32, [C.POINTER(vp), vp, u64, vp, u64, i32, i32]),
    "granne_hip_index_load_files": (i32, [C.POINTER(vp), C.c_char_p, C.c_char_p, i32, i32]),
    "granne_hip_write_index_file": (i32, [C.c_char_p, u32, vp, vp, vp]),
    "granne_hip_write_elements_file": (i32, [C.c_char_p, vp, u64, u32, i32]),
    "granne_hip_index_save": (i32, [vp, C.c_char_p, C.c_char_p]),
    "granne_hip_index_encode": (i32, [vp, C.POINTER(vp), C.POINTER(u64)]),
    "granne_hip_bytes_free": (None, [vp]),
    "granne_hip_index_encode_on_device": (i32, [vp, u64, C.POINTER(vp), C.POINTER(u64), vp]),
    "granne_hip_index_save_on_device": (i32, [vp, C.c_char_p, C.c_char_p, u64, vp]),
    "granne_hip_index_load_on_device": (i32, [C.POINTER(vp), vp, u64, vp, u64, i32, i32, u64, vp]),
    "granne_hip_index_load_files_on_device": (i32, [C.POINTER(vp), C.c_char_p, C.c_char_p, i32, i32, u64, vp]),
    "granne_hip_index_file_info": (i32, [vp, u64, C.POINTER(u32), vp, vp, u32]),
    "granne_hip_index_file_decode_layer": (i32, [vp, u64, u32, vp, vp]),
    "granne_hip_brute_force_device": (i32, [vp, vp, u32, u32, vp, vp, vp, vp]),
    "granne_hip_brute_force": (i32, [vp, vp, u32, u32, vp, vp, vp]),
    "granne_hip_exact_topk_device": (i32, [vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_exact_topk": (i32, [vp, vp, u32, u32, vp, vp, vp, vp]),
    "granne_hip_merge_topk_device": (i32, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, i32, vp]),
    "granne_hip_packed_topk_bytes": (u64, [u32, u32]),
    "granne_hip_search_batch_packed_device": (i32, [vp, vp, u32, u32, u32, vp, vp, vp]),
    "granne_hip_merge_topk_packed_device": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, i32, vp]),
    "granne_hip_merge_topk_packed_strided_device": (i32, [vp, u64, vp, u32, u32, u32, vp, vp, vp, i32, vp]),
    "granne_hip_sharded_create": (i32, [C.POINTER(vp), vp, vp, u32]),
    "granne_hip_sharded_create_grouped": (i32, [C.POINTER(vp), vp, vp, u32, vp]),
    "granne_hip_sharded_destroy": (None, [vp]),
    "granne_hip_sharded_num_shards": (u32, [vp]),
    "granne_hip_sharded_len": (u64, [vp]),
    "granne_hip_sharded_device": (i32, [vp]),
    "granne_hip_sharded_shard": (vp, [vp, u32]),
    "granne_hip_sharded_shard_offset": (u64, [vp, u32]),
    "granne_hip_sharded_build": (i32, [C.POINTER(vp), vp, vp, u64, u32, i32, u32, vp, u32]),
    "granne_hip_sharded_set_option": (i32, [vp, i32, u64]),
    "granne_hip_sharded_get_option": (i32, [vp, i32, C.POINTER(u64)]),
    "granne_hip_sharded_search_batch_device": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_sharded_begin_device": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, C.POINTER(u64)]),
    "granne_hip_sharded_end_device": (i32, [vp, u64, vp]),
    "granne_hip_sharded_search_batches": (i32, [vp, vp, u32, u32, u32, u32, vp, vp, vp]),
    "granne_hip_sharded_search_batch": (i32, [vp, vp, u32, u32, u32, vp, vp, vp]),
    "granne_hip_sharded_search": (i32, [vp, vp, u32, u32, vp, vp, C.POINTER(u32)]),
    "granne_hip_build_config_default": (None, [vp]),
    "granne_hip_builder_create": (i32, [C.POINTER(vp), vp, vp, u64, u32, i32, i32]),
    "granne_hip_builder_create_device": (i32, [C.POINTER(vp), vp, vp, u64, u32, i32, i32, vp]),
    "granne_hip_builder_append": (i32, [vp, vp, u64]),
    "granne_hip_builder_load_index": (i32, [vp, vp, u64]),
    "granne_hip_builder_build": (i32, [vp, u64]),
    "granne_hip_builder_len": (u64, [vp]),
    "granne_hip_builder_num_elements": (u64, [vp]),
    "granne_hip_builder_num_layers": (u32, [vp]),
    "granne_hip_builder_layer_len": (u64, [vp, u32]),
    "granne_hip_builder_get_layer": (i32, [vp, u32, vp]),
    "granne_hip_builder_get_index": (i32, [vp, C.POINTER(vp)]),
    "granne_hip_builder_destroy": (None, [vp]),
    "granne_hip_index_set_option": (i32, [vp, i32, u64]),
    "granne_hip_index_get_option": (i32, [vp, i32, C.POINTER(u64)]),
    "granne_hip_index_last_slow_count": (u64, [vp]),
    "granne_hip_sum_embeddings_create": (i32, [C.POINTER(vp), vp, u64, u32, vp, vp, u64, i32]),
    "granne_hip_sum_embeddings_create_device": (i32, [C.POINTER(vp), vp, u64, u32, vp, vp, u64, i32, vp]),
    "granne_hip_sum_embeddings_load_files": (i32, [C.POINTER(vp), C.c_char_p, C.c_char_p, i32]),
    "granne_hip_sum_embeddings_load": (i32, [C.POINTER(vp), vp, u64, u32, vp, u64, i32]),
    "granne_hip_sum_embeddings_save_elements": (i32, [vp, C.c_char_p]),
    "granne_hip_sum_embeddings_save_embeddings": (i32, [vp, C.c_char_p]),
    "granne_hip_sum_embeddings_destroy": (None, [vp]),
    "granne_hip_sum_embeddings_len": (u64, [vp]),
    "granne_hip_sum_embeddings_num_embeddings": (u64, [vp]),
    "granne_hip_sum_embeddings_dim": (u32, [vp]),
    "granne_hip_sum_embeddings_hbm_bytes": (u64, [vp]),
    "granne_hip_sum_embeddings_get_terms": (i32, [vp, u64, vp, u32, C.POINTER(u32)]),
    "granne_hip_sum_embeddings_append": (i32, [vp, vp, vp, u64]),
    "granne_hip_sum_embeddings_materialize_device": (i32, [vp, u64, u64, i32, vp, u64, vp]),
    "granne_hip_sum_embeddings_materialize": (i32, [vp, u64, u64, i32, vp]),
    "granne_hip_sum_embeddings_embed_device": (i32, [vp, vp, vp, u64, i32, vp, u64, vp]),
    "granne_hip_sum_embeddings_embed": (i32, [vp, vp, vp, u64, i32, vp]),
    "granne_hip_index_create_sum_embeddings": (i32, [C.POINTER(vp), vp, u32, vp, vp, vp, i32]),
    "granne_hip_index_load_files_sum_embeddings": (i32, [C.POINTER(vp), C.c_char_p, C.c_char_p, C.c_char_p, i32, i32]),
    "granne_hip_builder_create_sum_embeddings": (i32, [C.POINTER(vp), vp, vp]),
    "granne_hip_builder_get_index_compact": (i32, [vp, C.POINTER(vp)]),
    "granne_hip_refine_sum_embeddings_device": (i32, [vp, vp, u32, vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_search_refined_sum_embeddings_batch_device": (i32, [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search_refined_sum_embeddings_batch": (i32, [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_sum_embeddings_rows_device": (i32, [vp, u64, u64, i32, vp, u64, vp]),
    "granne_hip_sum_embeddings_rows": (i32, [vp, u64, u64, i32, vp]),
    "granne_hip_rw_builder_create": (i32, [C.POINTER(vp), vp, u64]),
    "granne_hip_rw_builder_destroy": (None, [vp]),
    "granne_hip_rw_builder_insert_batch": (i32, [vp, vp, u64, vp, C.POINTER(u64)]),
    "granne_hip_rw_builder_search_batch": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp]),
    "granne_hip_rw_builder_search": (i32, [vp, vp, u32, u32, vp, vp, C.POINTER(u32)]),
    "granne_hip_rw_builder_len": (u64, [vp]),
    "granne_hip_rw_builder_max_elements": (u64, [vp]),
    "granne_hip_rw_builder_num_layers": (u32, [vp]),
    "granne_hip_rw_builder_layer_len": (u64, [vp, u32]),
    "granne_hip_rw_builder_get_layer": (i32, [vp, u32, vp]),
    "granne_hip_rw_builder_get_element": (i32, [vp, u64, vp]),
    "granne_hip_rw_builder_save": (i32, [vp, C.c_char_p, C.c_char_p]),
    "granne_hip_rw_builder_get_index": (i32, [vp, C.POINTER(vp)]),
    "granne_hip_rw_builder_set_option": (i32, [vp, i32, u64]),
    "granne_hip_rw_builder_get_option": (i32, [vp, i32, C.POINTER(u64)]),
    "granne_hip_rw_builder_remove": (i32, [vp, vp, u64, vp]),
    "granne_hip_rw_builder_restore": (i32, [vp, vp, u64, vp]),
    "granne_hip_rw_builder_removed_count": (u64, [vp]),
    "granne_hip_rw_builder_alive": (i32, [vp, vp, vp]),
    "granne_hip_rw_builder_compact": (i32, [vp, u64, C.POINTER(vp), vp, C.POINTER(u64)]),
    "granne_hip_search_filtered_batch_device": (i32, [vp, vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search_filtered_batch": (i32, [vp, vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp]),
    "granne_hip_filter_words": (i32, [u64, C.POINTER(u64)]),
    "granne_hip_filter_from_ids_device": (i32, [vp, u64, u64, vp, vp, i32, vp]),
    "granne_hip_filter_from_mask_device": (i32, [vp, u64, vp, i32, vp]),
    "granne_hip_filter_count_device": (i32, [vp, u64, vp, i32, vp]),
    "granne_hip_filter_to_ids_device": (i32, [vp, u64, vp, vp, i32, vp]),
    "granne_hip_exact_topk_filtered_device": (i32, [vp, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]),
    "granne_hip_exact_topk_filtered": (i32, [vp, vp, u32, u32, vp, u64, vp, vp, vp, vp]),
    "granne_hip_search_postfiltered_batch_device": (i32, [vp, vp, u32, u32, u32, vp, u32, i32, vp, u64, u64, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search_postfiltered_batch": (i32, [vp, vp, u32, u32, u32, vp, u32, i32, vp, u64, u64, vp, vp, vp, vp, vp]),
    "granne_hip_exact_range_device": (i32, [vp, vp, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp]),
    "granne_hip_exact_range": (i32, [vp, vp, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp]),
    "granne_hip_search_range_batch_device": (i32, [vp, vp, u32, vp, u32, vp, u32, i32, u64, vp, vp, vp, vp, vp, vp, vp]),
    "granne_hip_search_range_batch": (i32, [vp, vp, u32, vp, u32, vp, u32, i32, u64, vp, vp, vp, vp, vp, vp]),
    "granne_hip_filter_slice_device": (i32, [vp, u64, u64, u32, u64, u64, vp, u64, i32, vp]),
    "granne_hip_sharded_id_span": (u64, [vp]),
    "granne_hip_sharded_search_filtered_batch_device": (i32, [vp, vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp]),
    "granne_hip_sharded_search_filtered_batch": (i32, [vp, vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk_device": (i32, [vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk": (i32, [vp, vp, u32, u32, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk_filtered_device": (i32, [vp, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk_filtered": (i32, [vp, vp, u32, u32, vp, u64, vp, vp, vp, vp]),
}


def lib():
    """The loaded library. Raises if it has not been built (python -m granne_amd.build)."""
    global _lib
    if _lib is None:
        path = os.environ.get("GRANNE_HIP_LIB") or _build.LIB_PATH  # GRANNE_HIP_LIB: kernel experiments (tools/sweep.py)
        if not os.path.exists(path):
            raise GranneHipError(ERR_NO_DEVICE, "libgranne_hip.so is not built: run `python -m granne_amd.build` "
                                 "(no CPU fallback exists)")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64. If torch is
        # importable, load it first so that libgranne_hip.so binds to the same runtime (two
        # runtimes in one process leave the second without devices).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise GranneHipError(rc, lib().granne_hip_last_error().decode("utf-8", "replace"))
    return rc
