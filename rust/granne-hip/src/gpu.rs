//! MI355X back end for `Granne::search` (feature "hip"): the index lives in HBM, the walk runs in
//! libgranne_hip.so. Results equal `Granne::search` bit for bit (ids, distances, order).
use crate::{angular, angular_int, Index};
use std::marker::PhantomData;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct granne_hip_index { _private: [u8; 0] }
#[repr(C)] pub struct granne_hip_builder { _private: [u8; 0] }
#[repr(C)] pub struct granne_hip_sharded { _private: [u8; 0] }
#[repr(C)] pub struct granne_hip_sum_embeddings { _private: [u8; 0] }
#[repr(C)] pub struct granne_hip_rw_builder { _private: [u8; 0] }

pub const GRANNE_HIP_F32: c_int = 0;
pub const GRANNE_HIP_I8: c_int = 1;
/// rows of IEEE halves, normalised where they are read ("angular_f16"); queries are prepared f32 rows
pub const GRANNE_HIP_F16: c_int = 2;
pub const GRANNE_HIP_BUILD_ALL: u64 = u64::MAX;

/// `granne_hip_build_config` (include/granne_hip.h) = `BuildConfig` (src/index/mod.rs:198-231)
/// + the GPU builder's batch schedule.
#[repr(C)]
pub struct granne_hip_build_config {
    pub layer_multiplier: f32,
    pub expected_num_elements: u64,
    pub num_neighbors: u32,
    pub max_search: u32,
    pub reinsert_elements: c_int,
    pub show_progress: c_int,
    pub batch_max: u32,
    pub batch_div: u32,
}

extern "C" {
    fn granne_hip_last_error() -> *const c_char;
    fn granne_hip_device_count(out_count: *mut c_int) -> c_int;
    // ---- index
    fn granne_hip_index_create(out: *mut *mut granne_hip_index, elements: *const c_void, n_elements: u64,
        dim: u32, dtype: c_int, n_layers: u32, layer_len: *const u64,
        layer_rows: *const *const u32, layer_width: *const u32, device_id: c_int) -> c_int;
    fn granne_hip_index_create_csr(out: *mut *mut granne_hip_index, elements: *const c_void, n_elements: u64,
        dim: u32, dtype: c_int, n_layers: u32, layer_len: *const u64,
        layer_offsets: *const *const u64, layer_ids: *const *const u32, device_id: c_int) -> c_int;
    // Granne::from_bytes / from_file (src/index/mod.rs:108-137): granne's own index + elements files
    fn granne_hip_index_load(out: *mut *mut granne_hip_index, index_bytes: *const c_void, index_len: u64,
        elements_bytes: *const c_void, elements_len: u64, dtype: c_int, device_id: c_int) -> c_int;
    fn granne_hip_index_load_files(out: *mut *mut granne_hip_index, index_path: *const c_char,
        elements_path: *const c_char, dtype: c_int, device_id: c_int) -> c_int;
    fn granne_hip_index_save(index: *const granne_hip_index, index_path: *const c_char, elements_path: *const c_char) -> c_int;
    fn granne_hip_index_encode(index: *const granne_hip_index, out_bytes: *mut *mut c_void, out_len: *mut u64) -> c_int;
    fn granne_hip_bytes_free(bytes: *mut c_void);
    // the same files through the device codec (granne_amd/csrc/codec_kernels.h), streamed through a pinned ring
    fn granne_hip_index_encode_on_device(index: *const granne_hip_index, staging_bytes: u64,
        out_bytes: *mut *mut c_void, out_len: *mut u64, out_info: *mut u64) -> c_int;
    fn granne_hip_index_save_on_device(index: *const granne_hip_index, index_path: *const c_char,
        elements_path: *const c_char, staging_bytes: u64, out_info: *mut u64) -> c_int;
    fn granne_hip_index_load_on_device(out: *mut *mut granne_hip_index, index_bytes: *const c_void, index_len: u64,
        elements_bytes: *const c_void, elements_len: u64, dtype: c_int, device_id: c_int, staging_bytes: u64,
        out_info: *mut u64) -> c_int;
    fn granne_hip_index_load_files_on_device(out: *mut *mut granne_hip_index, index_path: *const c_char,
        elements_path: *const c_char, dtype: c_int, device_id: c_int, staging_bytes: u64, out_info: *mut u64) -> c_int;
    fn granne_hip_index_destroy(index: *mut granne_hip_index);
    fn granne_hip_index_len(index: *const granne_hip_index) -> u64;
    fn granne_hip_index_num_elements(index: *const granne_hip_index) -> u64;
    fn granne_hip_index_num_layers(index: *const granne_hip_index) -> u32;
    fn granne_hip_index_layer_len(index: *const granne_hip_index, layer: u32) -> u64;
    fn granne_hip_index_dim(index: *const granne_hip_index) -> u32;
    fn granne_hip_index_get_neighbors(index: *const granne_hip_index, node: u64, layer: u32,
        out_ids: *mut u32, cap: u32, out_count: *mut u32) -> c_int;
    fn granne_hip_index_get_element(index: *const granne_hip_index, idx: u64, out: *mut c_void) -> c_int;
    fn granne_hip_index_get_sketch(index: *const granne_hip_index, first: u64, count: u64, out: *mut c_void) -> c_int;
    // ---- search
    fn granne_hip_search(index: *const granne_hip_index, query: *const c_void, max_search: u32,
        num_neighbors: u32, out_ids: *mut u64, out_dists: *mut f32, out_count: *mut u32) -> c_int;
    fn granne_hip_search_batch(index: *const granne_hip_index, queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, out_ids: *mut u64, out_dists: *mut f32,
        out_counts: *mut u32, out_stats: *mut u64) -> c_int;
    // ---- refined search: walk one index, re-rank the candidates by another's rows
    fn granne_hip_refine_device(refine_index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        d_cand_ids: *const u64, d_cand_counts: *const u32, m: u32, k: u32, d_out_ids: *mut u64,
        d_out_dists: *mut f32, d_out_counts: *mut u32, d_refine_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_search_refined_batch_device(walk_index: *const granne_hip_index,
        refine_index: *const granne_hip_index, d_walk_queries: *const c_void, d_refine_queries: *const c_void,
        nq: u32, max_search: u32, refine_from: u32, k: u32, d_out_ids: *mut u64, d_out_dists: *mut f32,
        d_out_counts: *mut u32, d_out_stats: *mut u64, d_status: *mut u32, d_refine_status: *mut u32,
        stream: *mut c_void) -> c_int;
    fn granne_hip_search_refined_batch(walk_index: *const granne_hip_index, refine_index: *const granne_hip_index,
        walk_queries: *const c_void, refine_queries: *const c_void, nq: u32, max_search: u32, refine_from: u32,
        k: u32, out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32, out_stats: *mut u64,
        out_refine_status: *mut u32) -> c_int;
    // ---- Granne::reorder / reorder_by_keys (src/index/reorder.rs:59-133)
    fn granne_hip_index_reorder(index: *mut granne_hip_index, out_order: *mut u64) -> c_int;
    fn granne_hip_index_reorder_by_keys(index: *mut granne_hip_index, keys: *const u64, out_order: *mut u64) -> c_int;
    // ---- ElementContainer::dist_to_element for explicit pairs (src/elements/dense_vector.rs:149-163)
    fn granne_hip_dist_pairs(index: *const granne_hip_index, queries: *const c_void, nq: u32,
        qidx: *const u32, ids: *const u32, n_pairs: u64, out: *mut f32) -> c_int;
    // ---- GranneBuilder (src/index/mod.rs:295-531)
    fn granne_hip_build_config_default(config: *mut granne_hip_build_config);
    fn granne_hip_builder_create(out: *mut *mut granne_hip_builder, config: *const granne_hip_build_config,
        elements: *const c_void, n_elements: u64, dim: u32, dtype: c_int, device_id: c_int) -> c_int;
    fn granne_hip_builder_append(builder: *mut granne_hip_builder, elements: *const c_void, n_new: u64) -> c_int;
    fn granne_hip_builder_load_index(builder: *mut granne_hip_builder, index_bytes: *const c_void, index_len: u64) -> c_int;
    fn granne_hip_builder_build(builder: *mut granne_hip_builder, num_elements: u64) -> c_int;
    fn granne_hip_builder_len(builder: *const granne_hip_builder) -> u64;
    fn granne_hip_builder_num_layers(builder: *const granne_hip_builder) -> u32;
    fn granne_hip_builder_layer_len(builder: *const granne_hip_builder, layer: u32) -> u64;
    fn granne_hip_builder_get_layer(builder: *const granne_hip_builder, layer: u32, out_rows: *mut u32) -> c_int;
    fn granne_hip_builder_get_index(builder: *const granne_hip_builder, out: *mut *mut granne_hip_index) -> c_int;
    fn granne_hip_builder_destroy(builder: *mut granne_hip_builder);
    // ---- partitioned index, one host process (device_ids / n_devices / partitioned)
    fn granne_hip_sharded_create(out: *mut *mut granne_hip_sharded, shards: *const *mut granne_hip_index,
        id_offsets: *const u64, n_shards: u32) -> c_int;
    fn granne_hip_sharded_create_grouped(out: *mut *mut granne_hip_sharded, shards: *const *mut granne_hip_index,
        id_offsets: *const u64, n_shards: u32, groups: *const u32) -> c_int;
    fn granne_hip_sharded_destroy(sharded: *mut granne_hip_sharded);
    fn granne_hip_sharded_len(sharded: *const granne_hip_sharded) -> u64;
    fn granne_hip_sharded_search_batch(sharded: *mut granne_hip_sharded, queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32) -> c_int;
    fn granne_hip_sharded_search_batches(sharded: *mut granne_hip_sharded, queries: *const c_void, n_batches: u32,
        nq: u32, max_search: u32, num_neighbors: u32, out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32) -> c_int;
    fn granne_hip_sharded_set_option(sharded: *mut granne_hip_sharded, option: c_int, value: u64) -> c_int;
    fn granne_hip_sharded_build(out: *mut *mut granne_hip_sharded, config: *const granne_hip_build_config,
        elements: *const c_void, n_elements: u64, dim: u32, dtype: c_int, n_shards: u32, device_ids: *const c_int,
        n_devices: u32) -> c_int;
    // ---- embeddings::SumEmbeddings: the container, its files, materialised and compact indexes
    fn granne_hip_sum_embeddings_create(out: *mut *mut granne_hip_sum_embeddings, table: *const f32,
        n_embeddings: u64, dim: u32, offsets: *const u64, terms: *const u32, n_elements: u64, device_id: c_int) -> c_int;
    fn granne_hip_sum_embeddings_create_device(out: *mut *mut granne_hip_sum_embeddings, d_table: *const f32,
        n_embeddings: u64, dim: u32, d_offsets: *const u64, d_terms: *const u32, n_elements: u64, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_sum_embeddings_load_files(out: *mut *mut granne_hip_sum_embeddings,
        embeddings_path: *const c_char, elements_path: *const c_char, device_id: c_int) -> c_int;
    fn granne_hip_sum_embeddings_load(out: *mut *mut granne_hip_sum_embeddings, table: *const f32,
        n_embeddings: u64, dim: u32, elements_bytes: *const c_void, elements_len: u64, device_id: c_int) -> c_int;
    fn granne_hip_sum_embeddings_save_elements(se: *const granne_hip_sum_embeddings, path: *const c_char) -> c_int;
    fn granne_hip_sum_embeddings_save_embeddings(se: *const granne_hip_sum_embeddings, path: *const c_char) -> c_int;
    fn granne_hip_sum_embeddings_destroy(se: *mut granne_hip_sum_embeddings);
    fn granne_hip_sum_embeddings_len(se: *const granne_hip_sum_embeddings) -> u64;
    fn granne_hip_sum_embeddings_num_embeddings(se: *const granne_hip_sum_embeddings) -> u64;
    fn granne_hip_sum_embeddings_dim(se: *const granne_hip_sum_embeddings) -> u32;
    fn granne_hip_sum_embeddings_hbm_bytes(se: *const granne_hip_sum_embeddings) -> u64;
    fn granne_hip_sum_embeddings_get_terms(se: *const granne_hip_sum_embeddings, idx: u64, out_terms: *mut u32,
        cap: u32, out_count: *mut u32) -> c_int;
    fn granne_hip_sum_embeddings_append(se: *mut granne_hip_sum_embeddings, offsets: *const u64, terms: *const u32,
        n_new: u64) -> c_int;
    fn granne_hip_sum_embeddings_materialize_device(se: *const granne_hip_sum_embeddings, first: u64, count: u64,
        normalised: c_int, d_out: *mut f32, stride: u64, stream: *mut c_void) -> c_int;
    fn granne_hip_sum_embeddings_materialize(se: *const granne_hip_sum_embeddings, first: u64, count: u64,
        normalised: c_int, out: *mut f32) -> c_int;
    fn granne_hip_sum_embeddings_embed_device(se: *const granne_hip_sum_embeddings, d_offsets: *const u64,
        d_terms: *const u32, nq: u64, normalised: c_int, d_out: *mut f32, stride: u64, stream: *mut c_void) -> c_int;
    fn granne_hip_sum_embeddings_embed(se: *const granne_hip_sum_embeddings, offsets: *const u64,
        terms: *const u32, nq: u64, normalised: c_int, out: *mut f32) -> c_int;
    fn granne_hip_index_create_sum_embeddings(out: *mut *mut granne_hip_index,
        se: *const granne_hip_sum_embeddings, n_layers: u32, layer_len: *const u64, layer_rows: *const *const u32,
        layer_width: *const u32, mode: c_int) -> c_int;
    fn granne_hip_index_load_files_sum_embeddings(out: *mut *mut granne_hip_index, index_path: *const c_char,
        embeddings_path: *const c_char, elements_path: *const c_char, mode: c_int, device_id: c_int) -> c_int;
    fn granne_hip_builder_create_sum_embeddings(out: *mut *mut granne_hip_builder,
        config: *const granne_hip_build_config, se: *const granne_hip_sum_embeddings) -> c_int;
    fn granne_hip_builder_get_index_compact(builder: *const granne_hip_builder, out: *mut *mut granne_hip_index) -> c_int;
    // ---- refined search over a container: walk dense rows, re-rank by term sums; the container as prepared rows
    fn granne_hip_refine_sum_embeddings_device(se: *const granne_hip_sum_embeddings, d_queries: *const f32,
        nq: u32, d_cand_ids: *const u64, d_cand_counts: *const u32, m: u32, k: u32, d_out_ids: *mut u64,
        d_out_dists: *mut f32, d_out_counts: *mut u32, d_refine_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_search_refined_sum_embeddings_batch_device(walk_index: *const granne_hip_index,
        se: *const granne_hip_sum_embeddings, d_walk_queries: *const c_void, d_refine_queries: *const c_void,
        nq: u32, max_search: u32, refine_from: u32, k: u32, d_out_ids: *mut u64, d_out_dists: *mut f32,
        d_out_counts: *mut u32, d_out_stats: *mut u64, d_status: *mut u32, d_refine_status: *mut u32,
        stream: *mut c_void) -> c_int;
    fn granne_hip_search_refined_sum_embeddings_batch(walk_index: *const granne_hip_index,
        se: *const granne_hip_sum_embeddings, walk_queries: *const c_void, refine_queries: *const c_void, nq: u32,
        max_search: u32, refine_from: u32, k: u32, out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32,
        out_stats: *mut u64, out_refine_status: *mut u32) -> c_int;
    fn granne_hip_sum_embeddings_rows_device(se: *const granne_hip_sum_embeddings, first: u64, count: u64,
        dtype: c_int, d_out: *mut c_void, stride_bytes: u64, stream: *mut c_void) -> c_int;
    fn granne_hip_sum_embeddings_rows(se: *const granne_hip_sum_embeddings, first: u64, count: u64, dtype: c_int,
        out: *mut c_void) -> c_int;
    // ---- RwGranneBuilder (src/index/rw/mod.rs:15-224)
    fn granne_hip_rw_builder_create(out: *mut *mut granne_hip_rw_builder, builder: *mut granne_hip_builder,
        max_elements: u64) -> c_int;
    fn granne_hip_rw_builder_destroy(rw: *mut granne_hip_rw_builder);
    fn granne_hip_rw_builder_insert_batch(rw: *mut granne_hip_rw_builder, rows: *const c_void, n_new: u64,
        out_ids: *mut u64, out_count: *mut u64) -> c_int;
    fn granne_hip_rw_builder_search_batch(rw: *mut granne_hip_rw_builder, queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32,
        out_stats: *mut u64) -> c_int;
    fn granne_hip_rw_builder_search(rw: *mut granne_hip_rw_builder, query: *const c_void, max_search: u32,
        num_neighbors: u32, out_ids: *mut u64, out_dists: *mut f32, out_count: *mut u32) -> c_int;
    fn granne_hip_rw_builder_len(rw: *mut granne_hip_rw_builder) -> u64;
    fn granne_hip_rw_builder_max_elements(rw: *mut granne_hip_rw_builder) -> u64;
    fn granne_hip_rw_builder_num_layers(rw: *mut granne_hip_rw_builder) -> u32;
    fn granne_hip_rw_builder_layer_len(rw: *mut granne_hip_rw_builder, layer: u32) -> u64;
    fn granne_hip_rw_builder_get_layer(rw: *mut granne_hip_rw_builder, layer: u32, out_rows: *mut u32) -> c_int;
    fn granne_hip_rw_builder_get_element(rw: *mut granne_hip_rw_builder, idx: u64, out: *mut c_void) -> c_int;
    fn granne_hip_rw_builder_save(rw: *mut granne_hip_rw_builder, index_path: *const c_char,
        elements_path: *const c_char) -> c_int;
    fn granne_hip_rw_builder_get_index(rw: *mut granne_hip_rw_builder, out: *mut *mut granne_hip_index) -> c_int;
    fn granne_hip_rw_builder_set_option(rw: *mut granne_hip_rw_builder, option: c_int, value: u64) -> c_int;
    fn granne_hip_rw_builder_get_option(rw: *mut granne_hip_rw_builder, option: c_int, value: *mut u64) -> c_int;
    fn granne_hip_rw_builder_remove(rw: *mut granne_hip_rw_builder, ids: *const u64, n: u64, out_counts: *mut u64) -> c_int;
    fn granne_hip_rw_builder_restore(rw: *mut granne_hip_rw_builder, ids: *const u64, n: u64, out_counts: *mut u64) -> c_int;
    fn granne_hip_rw_builder_removed_count(rw: *mut granne_hip_rw_builder) -> u64;
    fn granne_hip_rw_builder_alive(rw: *mut granne_hip_rw_builder, d_filter_out: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_rw_builder_compact(rw: *mut granne_hip_rw_builder, max_elements: u64,
        out_rw: *mut *mut granne_hip_rw_builder, out_old_ids: *mut u64, out_count: *mut u64) -> c_int;
    // filtered search: the walk under an id bitmap; bitmaps
    fn granne_hip_search_filtered_batch_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_filter: *const u32, filter_stride_words: u64, max_expand: u64,
        d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32, d_out_stats: *mut u64,
        d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_search_filtered_batch(index: *const granne_hip_index, queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, filter: *const u32, filter_stride_words: u64, max_expand: u64,
        out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32, out_stats: *mut u64, out_status: *mut u32) -> c_int;
    fn granne_hip_filter_words(n_elements: u64, out_words: *mut u64) -> c_int;
    fn granne_hip_filter_from_ids_device(d_ids: *const u64, n_ids: u64, n_elements: u64, d_filter: *mut u32,
        d_bad: *mut u32, device_id: c_int, stream: *mut c_void) -> c_int;
    fn granne_hip_filter_from_mask_device(d_mask: *const u8, n_elements: u64, d_filter: *mut u32, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_filter_count_device(d_filter: *const u32, n_elements: u64, d_out: *mut u64, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_filter_to_ids_device(d_filter: *const u32, n_elements: u64, d_out_ids: *mut u64,
        d_out_count: *mut u64, device_id: c_int, stream: *mut c_void) -> c_int;
    // the exact scan under an id bitmap
    fn granne_hip_exact_topk_filtered_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        k: u32, d_filter: *const u32, filter_stride_words: u64, d_out_ids: *mut u64, d_out_dists: *mut f32,
        d_out_counts: *mut u32, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_exact_topk_filtered(index: *const granne_hip_index, queries: *const c_void, nq: u32, k: u32,
        filter: *const u32, filter_stride_words: u64, out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32,
        out_status: *mut u32) -> c_int;
    // partitioned indexes: the bitmap slice, filtered search and the exact selection over global ids
    fn granne_hip_filter_slice_device(d_filter: *const u32, n_bits: u64, filter_stride_words: u64, n_filters: u32,
        first_bit: u64, n_out_bits: u64, d_out: *mut u32, out_stride_words: u64, device_id: c_int, stream: *mut c_void) -> c_int;
    fn granne_hip_sharded_id_span(sharded: *const granne_hip_sharded) -> u64;
    fn granne_hip_sharded_search_filtered_batch_device(sharded: *mut granne_hip_sharded, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_filter: *const u32, filter_stride_words: u64, max_expand: u64,
        d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_sharded_search_filtered_batch(sharded: *mut granne_hip_sharded, queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, filter: *const u32, filter_stride_words: u64, max_expand: u64,
        out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32, out_status: *mut u32) -> c_int;
    fn granne_hip_sharded_exact_topk_device(sharded: *mut granne_hip_sharded, d_queries: *const c_void, nq: u32, k: u32,
        d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_sharded_exact_topk(sharded: *mut granne_hip_sharded, queries: *const c_void, nq: u32, k: u32,
        out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32, out_status: *mut u32) -> c_int;
    fn granne_hip_sharded_exact_topk_filtered_device(sharded: *mut granne_hip_sharded, d_queries: *const c_void, nq: u32,
        k: u32, d_filter: *const u32, filter_stride_words: u64, d_out_ids: *mut u64, d_out_dists: *mut f32,
        d_out_counts: *mut u32, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_sharded_exact_topk_filtered(sharded: *mut granne_hip_sharded, queries: *const c_void, nq: u32, k: u32,
        filter: *const u32, filter_stride_words: u64, out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32,
        out_status: *mut u32) -> c_int;
    // post-filtered search: staged over-fetch on the ordinary search
    fn granne_hip_search_postfiltered_batch_device(index: *const granne_hip_index, d_queries: *const c_void,
        nq: u32, num_neighbors: u32, min_allowed: u32, stages: *const u32, n_stages: u32, fallback: c_int,
        d_filter: *const u32, filter_stride_words: u64, scratch_bytes: u64, d_out_ids: *mut u64,
        d_out_dists: *mut f32, d_out_counts: *mut u32, d_out_stage: *mut u32, d_status: *mut u32,
        stream: *mut c_void) -> c_int;
    fn granne_hip_search_postfiltered_batch(index: *const granne_hip_index, queries: *const c_void, nq: u32,
        num_neighbors: u32, min_allowed: u32, stages: *const u32, n_stages: u32, fallback: c_int,
        filter: *const u32, filter_stride_words: u64, scratch_bytes: u64, out_ids: *mut u64, out_dists: *mut f32,
        out_counts: *mut u32, out_stage: *mut u32, out_status: *mut u32) -> c_int;
    // range search: all elements within a radius, by the exact scan and by the staged walk
    fn granne_hip_exact_range_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        d_radii: *const f32, cap: u32, d_filter: *const u32, filter_stride_words: u64, d_out_ids: *mut u64,
        d_out_dists: *mut f32, d_out_counts: *mut u32, d_out_totals: *mut u32, d_status: *mut u32,
        stream: *mut c_void) -> c_int;
    fn granne_hip_exact_range(index: *const granne_hip_index, queries: *const c_void, nq: u32, radii: *const f32,
        cap: u32, filter: *const u32, filter_stride_words: u64, out_ids: *mut u64, out_dists: *mut f32,
        out_counts: *mut u32, out_totals: *mut u32, out_status: *mut u32) -> c_int;
    fn granne_hip_search_range_batch_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        d_radii: *const f32, cap: u32, stages: *const u32, n_stages: u32, fallback: c_int, scratch_bytes: u64,
        d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32, d_out_found: *mut u32,
        d_out_stage: *mut u32, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_search_range_batch(index: *const granne_hip_index, queries: *const c_void, nq: u32,
        radii: *const f32, cap: u32, stages: *const u32, n_stages: u32, fallback: c_int, scratch_bytes: u64,
        out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32, out_found: *mut u32, out_stage: *mut u32,
        out_status: *mut u32) -> c_int;
}
pub const GRANNE_HIP_RANGE_CAP_MAX: usize = 1024;
pub const GRANNE_HIP_RG_MAX_STAGES: usize = 8;
pub const GRANNE_HIP_RG_FALLBACK_SHORT: c_int = 0;
pub const GRANNE_HIP_RG_FALLBACK_EXACT: c_int = 1;
pub const GRANNE_HIP_RG_STAGE_EXACT: u32 = 0xFFFF_FFFF;
pub const GRANNE_HIP_RG_STAGE_SHORT: u32 = 0xFFFF_FFFE;
pub const GRANNE_HIP_PF_MAX_STAGES: usize = 8;
pub const GRANNE_HIP_PF_FALLBACK_SHORT: c_int = 0;
pub const GRANNE_HIP_PF_FALLBACK_EXACT: c_int = 1;
pub const GRANNE_HIP_PF_STAGE_EXACT: u32 = 0xFFFF_FFFF;
pub const GRANNE_HIP_PF_STAGE_SHORT: u32 = 0xFFFF_FFFE;
pub const GRANNE_HIP_OPT_SEARCH_DEPTH: c_int = 9;
pub const GRANNE_HIP_OPT_INLINE_TAILS: c_int = 10;
pub const GRANNE_HIP_OPT_SEEN_MIN: c_int = 11;
pub const GRANNE_HIP_OPT_SKETCH: c_int = 12;
pub const GRANNE_HIP_OPT_COALESCE: c_int = 13;
pub const GRANNE_HIP_OPT_COALESCE_MAX: c_int = 14;
pub const GRANNE_HIP_OPT_COALESCE_WAIT_US: c_int = 15;
pub const GRANNE_HIP_OPT_COALESCED_LAUNCHES: c_int = 16;
pub const GRANNE_HIP_OPT_COALESCED_QUERIES: c_int = 17;
pub const GRANNE_HIP_OPT_LAST_COMPACT_ROWS: c_int = 18;
pub const GRANNE_HIP_OPT_LAST_SPLIT_TAIL: c_int = 19;
pub const GRANNE_HIP_OPT_LAST_SCAN: c_int = 20;
pub const GRANNE_HIP_OPT_FORCE_GENERAL: c_int = 21;
pub const GRANNE_HIP_RW_OPT_SMALL_OPS: c_int = 1;
pub const GRANNE_HIP_RW_OPT_REMOVED: c_int = 4;
pub const GRANNE_HIP_RW_OPT_FILTERED_SEARCHES: c_int = 5;
pub const GRANNE_HIP_SHARDED_OPT_DEPTH: c_int = 1;
pub const GRANNE_HIP_SHARDED_OPT_EXCHANGE: c_int = 2;
pub const GRANNE_HIP_SHARDED_EXCHANGE_PEER: u64 = 0;
pub const GRANNE_HIP_SHARDED_EXCHANGE_RCCL: u64 = 1;

// The rest of the C ABI (include/granne_hip.h), not used by the wrappers below: generated from the header by
// tools/gen_rust_sys.py; tests/test_abi.py checks that every entry point is declared here exactly as the header has it.
extern "C" {
    // ---- library / handle queries
    fn granne_hip_abi_version() -> c_int;
    fn granne_hip_index_dtype(index: *const granne_hip_index) -> c_int;
    fn granne_hip_index_device(index: *const granne_hip_index) -> c_int;
    fn granne_hip_index_hbm_bytes(index: *const granne_hip_index) -> u64;
    fn granne_hip_index_last_slow_count(index: *const granne_hip_index) -> u64;
    fn granne_hip_index_set_option(index: *mut granne_hip_index, option: c_int, value: u64) -> c_int;
    fn granne_hip_index_get_option(index: *const granne_hip_index, option: c_int, value: *mut u64) -> c_int;
    fn granne_hip_builder_num_elements(builder: *const granne_hip_builder) -> u64;
    fn granne_hip_sharded_num_shards(sharded: *const granne_hip_sharded) -> u32;
    fn granne_hip_sharded_search(sharded: *mut granne_hip_sharded, query: *const c_void, max_search: u32,
        num_neighbors: u32, out_ids: *mut u64, out_dists: *mut f32, out_count: *mut u32) -> c_int;
    fn granne_hip_sharded_device(sharded: *const granne_hip_sharded) -> c_int;
    fn granne_hip_sharded_shard(sharded: *const granne_hip_sharded, shard: u32) -> *mut granne_hip_index;
    fn granne_hip_sharded_shard_offset(sharded: *const granne_hip_sharded, shard: u32) -> u64;
    fn granne_hip_sharded_get_option(sharded: *const granne_hip_sharded, option: c_int, value: *mut u64) -> c_int;
    // ---- Vector::from for whole arrays (src/elements/angular.rs:55-61, angular_int.rs:27-45), host buffers
    fn granne_hip_normalize_f32(rows: *mut f32, n: u64, dim: u32, device_id: c_int) -> c_int;
    fn granne_hip_quantize_f32(rows: *const f32, out: *mut i8, n: u64, dim: u32, device_id: c_int) -> c_int;
    // ---- GRANNE_HIP_F16 rows: f32 -> halves (round to nearest even), halves -> f32 (exact, optionally Vector::from)
    fn granne_hip_f32_to_f16(rows: *const f32, out: *mut u16, n: u64, dim: u32, device_id: c_int) -> c_int;
    fn granne_hip_f16_to_f32(rows16: *const u16, out: *mut f32, n: u64, dim: u32, normalised: c_int,
        device_id: c_int) -> c_int;
    fn granne_hip_f32_to_f16_device(d_rows: *const f32, d_out: *mut u16, n: u64, dim: u32, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_f16_to_f32_device(d_rows16: *const u16, d_out: *mut f32, n: u64, dim: u32, normalised: c_int,
        device_id: c_int, stream: *mut c_void) -> c_int;
    // ---- granne's files without an index handle (src/index/io.rs:11-113, src/slice_vector/mod.rs:460-466)
    fn granne_hip_write_index_file(path: *const c_char, n_layers: u32, layer_len: *const u64,
        layer_rows: *const *const u32, layer_width: *const u32) -> c_int;
    fn granne_hip_write_elements_file(path: *const c_char, elements: *const c_void, n_elements: u64, dim: u32,
        dtype: c_int) -> c_int;
    fn granne_hip_index_file_info(index_bytes: *const c_void, index_len: u64, out_n_layers: *mut u32,
        out_layer_len: *mut u64, out_layer_ids: *mut u64, cap: u32) -> c_int;
    fn granne_hip_index_file_decode_layer(index_bytes: *const c_void, index_len: u64, layer: u32,
        out_offsets: *mut u64, out_ids: *mut u32) -> c_int;
    // ---- device-pointer entry points: for a host that already holds HIP memory and a hipStream_t (stream: *mut c_void); asynchronous
    fn granne_hip_index_create_device(out: *mut *mut granne_hip_index, d_elements: *const c_void, n_elements: u64,
        dim: u32, dtype: c_int, n_layers: u32, layer_len: *const u64, d_layer_rows: *const *const u32,
        layer_width: *const u32, device_id: c_int, stream: *mut c_void) -> c_int;
    fn granne_hip_builder_create_device(out: *mut *mut granne_hip_builder, config: *const granne_hip_build_config,
        d_elements: *const c_void, n_elements: u64, dim: u32, dtype: c_int, device_id: c_int, stream: *mut c_void) -> c_int;
    fn granne_hip_search_batch_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32,
        d_out_stats: *mut u64, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_search_batches_device(index: *const granne_hip_index, n_batches: u32,
        d_queries: *const *const c_void, nq: u32, max_search: u32, num_neighbors: u32, d_out_ids: *const *mut u64,
        d_out_dists: *const *mut f32, d_out_counts: *const *mut u32, d_out_stats: *const *mut u64,
        d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_search_begin_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32,
        d_out_stats: *mut u64, d_status: *mut u32, stream: *mut c_void, out_ticket: *mut u64) -> c_int;
    fn granne_hip_search_end_device(index: *const granne_hip_index, ticket: u64, stream: *mut c_void) -> c_int;
    // ---- device memory and streams for a host without HIP bindings of its own (DeviceBuffer / Stream below)
    fn granne_hip_device_malloc(out_ptr: *mut *mut c_void, bytes: u64, device_id: c_int) -> c_int;
    fn granne_hip_device_free(ptr: *mut c_void, device_id: c_int) -> c_int;
    fn granne_hip_copy_to_device(d_dst: *mut c_void, src: *const c_void, bytes: u64, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_copy_to_host(dst: *mut c_void, d_src: *const c_void, bytes: u64, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_stream_create(out_stream: *mut *mut c_void, device_id: c_int) -> c_int;
    fn granne_hip_stream_destroy(stream: *mut c_void, device_id: c_int) -> c_int;
    fn granne_hip_stream_synchronize(stream: *mut c_void, device_id: c_int) -> c_int;
    fn granne_hip_sharded_search_batch_device(sharded: *mut granne_hip_sharded, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32,
        d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_sharded_begin_device(sharded: *mut granne_hip_sharded, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32,
        d_status: *mut u32, stream: *mut c_void, out_ticket: *mut u64) -> c_int;
    fn granne_hip_sharded_end_device(sharded: *mut granne_hip_sharded, ticket: u64, stream: *mut c_void) -> c_int;
    fn granne_hip_search_batch_device_timed(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32,
        d_out_stats: *mut u64, d_status: *mut u32, stream: *mut c_void, ev_before: *mut c_void,
        ev_after: *mut c_void) -> c_int;
    fn granne_hip_search_batch_packed_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        max_search: u32, num_neighbors: u32, d_packed: *mut c_void, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_packed_topk_bytes(nq: u32, k: u32) -> u64;
    fn granne_hip_brute_force_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32, k: u32,
        d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_brute_force(index: *const granne_hip_index, queries: *const c_void, nq: u32, k: u32,
        out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32) -> c_int;
    fn granne_hip_exact_topk_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32, k: u32,
        d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_exact_topk(index: *const granne_hip_index, queries: *const c_void, nq: u32, k: u32,
        out_ids: *mut u64, out_dists: *mut f32, out_counts: *mut u32, out_status: *mut u32) -> c_int;
    fn granne_hip_merge_topk_device(d_ids: *const u64, d_dists: *const f32, d_counts: *const u32,
        shard_offsets: *const u64, n_shards: u32, nq: u32, k: u32, d_out_ids: *mut u64, d_out_dists: *mut f32,
        d_out_counts: *mut u32, device_id: c_int, stream: *mut c_void) -> c_int;
    fn granne_hip_merge_topk_packed_device(d_packed: *const c_void, shard_offsets: *const u64, n_shards: u32,
        nq: u32, k: u32, d_out_ids: *mut u64, d_out_dists: *mut f32, d_out_counts: *mut u32, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_merge_topk_packed_strided_device(d_packed: *const c_void, stride_bytes: u64,
        shard_offsets: *const u64, n_shards: u32, nq: u32, k: u32, d_out_ids: *mut u64, d_out_dists: *mut f32,
        d_out_counts: *mut u32, device_id: c_int, stream: *mut c_void) -> c_int;
    fn granne_hip_dist_pairs_device(index: *const granne_hip_index, d_queries: *const c_void, d_qidx: *const u32,
        d_ids: *const u32, n_pairs: u64, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn granne_hip_dists_device(index: *const granne_hip_index, d_queries: *const c_void, nq: u32,
        d_ids: *const u32, m: u32, d_out: *mut f32, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn granne_hip_normalize_f32_device(d_rows: *mut f32, n: u64, dim: u32, device_id: c_int, stream: *mut c_void) -> c_int;
    fn granne_hip_quantize_f32_device(d_rows: *const f32, d_out: *mut i8, n: u64, dim: u32, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_synth_rows_device(d_out: *mut f32, seed: u64, row0: u64, n: u64, dim: u32, device_id: c_int,
        stream: *mut c_void) -> c_int;
    fn granne_hip_event_create(out_event: *mut *mut c_void) -> c_int;
    fn granne_hip_event_destroy(event: *mut c_void);
    fn granne_hip_event_elapsed_ms(before: *mut c_void, after: *mut c_void, out_ms: *mut f32) -> c_int;
}

fn check(rc: c_int) -> std::io::Result<()> {
    if rc == 0 { return Ok(()); }
    let msg = unsafe { std::ffi::CStr::from_ptr(granne_hip_last_error()) }.to_string_lossy().into_owned();
    Err(std::io::Error::new(std::io::ErrorKind::Other, format!("granne_hip {}: {}", rc, msg)))
}

pub fn device_count() -> usize {
    let mut n: c_int = 0;
    unsafe { granne_hip_device_count(&mut n) };
    n.max(0) as usize
}

/// What the two dense element containers share, as the library needs it: prepared scalars, row major.
pub trait GpuElements {
    type Vector;
    const DTYPE: c_int;
    fn scalars(&self) -> *const c_void;
    fn n(&self) -> usize;
    fn width(&self) -> usize;
    fn query_scalars(v: &Self::Vector) -> *const c_void;
    fn query_len(v: &Self::Vector) -> usize;
    fn append_query(buf: &mut Vec<u8>, v: &Self::Vector);
}
macro_rules! gpu_elements {
    ($m:ident, $scalar:ty, $dtype:expr) => {
        impl<'a> GpuElements for $m::Vectors<'a> {
            type Vector = $m::Vector<'static>;
            const DTYPE: c_int = $dtype;
            fn scalars(&self) -> *const c_void { self.as_slice().as_ptr() as *const c_void }
            fn n(&self) -> usize { self.len() }
            fn width(&self) -> usize { self.dim() }
            fn query_scalars(v: &Self::Vector) -> *const c_void { v.as_slice().as_ptr() as *const c_void }
            fn query_len(v: &Self::Vector) -> usize { v.len() }
            fn append_query(buf: &mut Vec<u8>, v: &Self::Vector) {
                let s = v.as_slice();
                buf.extend_from_slice(unsafe {
                    std::slice::from_raw_parts(s.as_ptr() as *const u8, s.len() * std::mem::size_of::<$scalar>())
                });
            }
        }
    };
}
gpu_elements!(angular, f32, GRANNE_HIP_F32);
gpu_elements!(angular_int, i8, GRANNE_HIP_I8);

/// Marker for "angular_f16" element sets: `dim` IEEE binary16 values per element (their bits as `u16`), the element
/// they stand for being `angular::Vector::from(widen(row))`. The reference has no such container, so there is no
/// `Vectors` type to implement `GpuElements` for: `rows_to_f16` / `rows_from_f16` convert on the device, and an F16
/// index is made through the C entry points with `AngularF16::DTYPE`; its queries are `angular::Vector`s.
pub struct AngularF16;
impl AngularF16 {
    pub const DTYPE: c_int = GRANNE_HIP_F16;
    /// f32 rows ([n][dim], dense) -> halves, rounded to nearest even
    pub fn rows_to_f16(rows: &[f32], dim: usize, device: i32) -> std::io::Result<Vec<u16>> {
        let n = if dim == 0 { 0 } else { rows.len() / dim };
        let mut out = vec![0u16; n * dim];
        check(unsafe { granne_hip_f32_to_f16(rows.as_ptr(), out.as_mut_ptr(), n as u64, dim as u32, device as c_int) })?;
        Ok(out)
    }
    /// halves -> the f32 rows they stand for (widened exactly; `normalised`: then `Vector::from`)
    pub fn rows_from_f16(rows16: &[u16], dim: usize, normalised: bool, device: i32) -> std::io::Result<Vec<f32>> {
        let n = if dim == 0 { 0 } else { rows16.len() / dim };
        let mut out = vec![0f32; n * dim];
        check(unsafe { granne_hip_f16_to_f32(rows16.as_ptr(), out.as_mut_ptr(), n as u64, dim as u32, normalised as c_int, device as c_int) })?;
        Ok(out)
    }
}

/// A `Granne` whose layers and elements live in the HBM of one MI355X.
pub struct GpuGranne<E: GpuElements> { handle: *mut granne_hip_index, dim: usize, _e: PhantomData<E> }
unsafe impl<E: GpuElements> Send for GpuGranne<E> {}
unsafe impl<E: GpuElements> Sync for GpuGranne<E> {} // granne_hip_search_batch is thread-safe on a shared index

impl<E: GpuElements> GpuGranne<E> {
    fn wrap(handle: *mut granne_hip_index) -> Self {
        Self { handle, dim: unsafe { granne_hip_index_dim(handle) } as usize, _e: PhantomData }
    }
    /// From a builder's parts: `GranneBuilder::get_index()` hands out FixWidth layers (mod.rs:483-488);
    /// `layers[i]` is the row-major u32 matrix of layer i, `width` = config.num_neighbors, UNUSED padded.
    pub fn from_fix_width(elements: &E, layers: &[&[u32]], width: usize, device: i32) -> std::io::Result<Self> {
        let lens: Vec<u64> = layers.iter().map(|l| (l.len() / width) as u64).collect();
        let rows: Vec<*const u32> = layers.iter().map(|l| l.as_ptr()).collect();
        let widths: Vec<u32> = vec![width as u32; layers.len()];
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_index_create(&mut h, elements.scalars(), elements.n() as u64,
            elements.width() as u32, E::DTYPE, layers.len() as u32, lens.as_ptr(), rows.as_ptr(), widths.as_ptr(), device) })?;
        Ok(Self::wrap(h))
    }
    /// From decoded `MultiSetVector` layers (`get_into`, src/slice_vector/set_vector.rs:65-69): CSR per layer.
    pub fn from_csr(elements: &E, offsets: &[&[u64]], ids: &[&[u32]], device: i32) -> std::io::Result<Self> {
        let lens: Vec<u64> = offsets.iter().map(|o| (o.len() - 1) as u64).collect();
        let po: Vec<*const u64> = offsets.iter().map(|o| o.as_ptr()).collect();
        let pi: Vec<*const u32> = ids.iter().map(|i| i.as_ptr()).collect();
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_index_create_csr(&mut h, elements.scalars(), elements.n() as u64,
            elements.width() as u32, E::DTYPE, offsets.len() as u32, lens.as_ptr(), po.as_ptr(), pi.as_ptr(), device) })?;
        Ok(Self::wrap(h))
    }
    /// `Granne::from_bytes(index, elements)` (src/index/mod.rs:108-117) with the ELEMENTS as file bytes too
    /// (`Vectors::from_bytes`, dense_vector.rs:50-66): the library decodes granne's formats itself.
    pub fn from_bytes(index: &[u8], elements_file: &[u8], device: i32) -> std::io::Result<Self> {
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_index_load(&mut h, index.as_ptr() as *const c_void, index.len() as u64,
            elements_file.as_ptr() as *const c_void, elements_file.len() as u64, E::DTYPE, device) })?;
        Ok(Self::wrap(h))
    }
    /// `Granne::from_file` (src/index/mod.rs:120-137): the files are mapped by the library, uploaded, unmapped.
    pub fn from_files(index_path: &std::path::Path, elements_path: &std::path::Path, device: i32) -> std::io::Result<Self> {
        use std::os::unix::ffi::OsStrExt;
        let ip = std::ffi::CString::new(index_path.as_os_str().as_bytes())?;
        let ep = std::ffi::CString::new(elements_path.as_os_str().as_bytes())?;
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_index_load_files(&mut h, ip.as_ptr(), ep.as_ptr(), E::DTYPE, device) })?;
        Ok(Self::wrap(h))
    }
    /// `from_files` through the device codec: the files are read in pieces into a pinned ring of `staging_bytes` (0: the
    /// library's default) and decoded on the GPU; the index equals `from_files`'. Returns the call's four info words
    /// (layers on the device codec, layers on the host codec, peak device scratch bytes, peak host staging bytes).
    pub fn from_files_on_device(index_path: &std::path::Path, elements_path: &std::path::Path, device: i32,
                                staging_bytes: u64) -> std::io::Result<(Self, [u64; 4])> {
        use std::os::unix::ffi::OsStrExt;
        let ip = std::ffi::CString::new(index_path.as_os_str().as_bytes())?;
        let ep = std::ffi::CString::new(elements_path.as_os_str().as_bytes())?;
        let mut h = std::ptr::null_mut();
        let mut info = [0u64; 4];
        check(unsafe { granne_hip_index_load_files_on_device(&mut h, ip.as_ptr(), ep.as_ptr(), E::DTYPE, device, staging_bytes, info.as_mut_ptr()) })?;
        Ok((Self::wrap(h), info))
    }
    /// `save` through the device codec: the same two files, encoded on the GPU and streamed through the pinned ring.
    pub fn save_on_device(&self, index_path: &std::path::Path, elements_path: &std::path::Path, staging_bytes: u64) -> std::io::Result<[u64; 4]> {
        use std::os::unix::ffi::OsStrExt;
        let ip = std::ffi::CString::new(index_path.as_os_str().as_bytes())?;
        let ep = std::ffi::CString::new(elements_path.as_os_str().as_bytes())?;
        let mut info = [0u64; 4];
        check(unsafe { granne_hip_index_save_on_device(self.handle, ip.as_ptr(), ep.as_ptr(), staging_bytes, info.as_mut_ptr()) })?;
        Ok(info)
    }
    /// `write_index` + `write_elements` (src/index/io.rs:11-70, slice_vector/mod.rs:460-466) to two files.
    pub fn save(&self, index_path: &std::path::Path, elements_path: &std::path::Path) -> std::io::Result<()> {
        use std::os::unix::ffi::OsStrExt;
        let ip = std::ffi::CString::new(index_path.as_os_str().as_bytes())?;
        let ep = std::ffi::CString::new(elements_path.as_os_str().as_bytes())?;
        check(unsafe { granne_hip_index_save(self.handle, ip.as_ptr(), ep.as_ptr()) })
    }

    /// Same contract as `Granne::search` (src/index/mod.rs:140-150).
    pub fn search(&self, element: &E::Vector, max_search: usize, num_neighbors: usize) -> Vec<(usize, f32)> {
        assert_eq!(E::query_len(element), self.dim);
        let (mut ids, mut ds) = (vec![0u64; num_neighbors], vec![0f32; num_neighbors]);
        let mut count = 0u32;
        // the reference panics on max_search == 0 (mod.rs:1019); the ABI returns an error code
        check(unsafe { granne_hip_search(self.handle, E::query_scalars(element), max_search as u32,
            num_neighbors as u32, ids.as_mut_ptr(), ds.as_mut_ptr(), &mut count) }).expect("granne_hip_search");
        (0..count as usize).map(|j| (ids[j] as usize, ds[j])).collect()
    }
    /// The batch form the GPU is built for: `elements.len()` independent searches in one launch.
    pub fn search_batch(&self, elements: &[E::Vector], max_search: usize, num_neighbors: usize) -> Vec<Vec<(usize, f32)>> {
        let nq = elements.len();
        let mut q = Vec::new();
        for e in elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut q, e); }
        let (mut ids, mut ds) = (vec![0u64; nq * num_neighbors], vec![0f32; nq * num_neighbors]);
        let mut counts = vec![0u32; nq];
        check(unsafe { granne_hip_search_batch(self.handle, q.as_ptr() as *const c_void, nq as u32,
            max_search as u32, num_neighbors as u32, ids.as_mut_ptr(), ds.as_mut_ptr(),
            counts.as_mut_ptr(), std::ptr::null_mut()) }).expect("granne_hip_search_batch");
        (0..nq).map(|i| (0..counts[i] as usize)
            .map(|j| (ids[i * num_neighbors + j] as usize, ds[i * num_neighbors + j])).collect()).collect()
    }
    /// `granne_hip_exact_topk`: the `k` (up to 1024) nearest elements of every query by a scan of all rows in the
    /// reference's own arithmetic, selected by (distance bits, id): the exact answer `search` approximates, ties
    /// included. An `Err` when a query overflowed the selection (thousands of copies of one row at its k-th distance).
    pub fn exact_topk(&self, elements: &[E::Vector], k: usize) -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = elements.len();
        let mut q = Vec::new();
        for e in elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut q, e); }
        let (mut ids, mut ds) = (vec![0u64; nq * k], vec![0f32; nq * k]);
        let mut counts = vec![0u32; nq];
        check(unsafe { granne_hip_exact_topk(self.handle, q.as_ptr() as *const c_void, nq as u32, k as u32,
            ids.as_mut_ptr(), ds.as_mut_ptr(), counts.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok((0..nq).map(|i| (0..counts[i] as usize).map(|j| (ids[i * k + j] as usize, ds[i * k + j])).collect()).collect())
    }
    /// `granne_hip_exact_topk_filtered_device`: `exact_topk` among the ids `filter` allows (one bitmap for all queries,
    /// over `num_elements()` ids): the scan walks the bitmap's id list, exact by construction -- the tool for a selective
    /// filter. A result holds fewer than `k` ids when fewer are allowed.
    pub fn exact_topk_filtered(&self, elements: &[E::Vector], k: usize, filter: &GpuFilter) -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = elements.len();
        if nq == 0 { return Ok(Vec::new()); }
        assert_eq!(filter.len(), self.num_elements());
        let stream = Stream::new(self.device())?;
        let q = self.upload_queries(elements, &stream)?;
        let out = DeviceResults::new(nq, k, self.device())?;
        check(unsafe { granne_hip_exact_topk_filtered_device(self.handle, q.ptr as *const c_void, nq as u32, k as u32,
            filter.words.ptr as *const u32, 0, out.ids.ptr, out.dists.ptr, out.counts.ptr, std::ptr::null_mut(), stream.raw) })?;
        out.to_host(nq, &stream)
    }
    /// `granne_hip_search_postfiltered_batch_device`: the `num_neighbors` nearest ids `filter` allows, by the ordinary
    /// search with lists of `stages[s]` entries and a filter of its result. A query is answered by the first stage whose
    /// list holds `min_allowed` allowed ids (or whose walk ran out of graph); what no stage finishes gets the exact scan
    /// under the filter (`GRANNE_HIP_PF_FALLBACK_EXACT`) or its short answer (`_SHORT`). The call waits on its stream once
    /// per stage it goes beyond.
    pub fn search_postfiltered(&self, elements: &[E::Vector], num_neighbors: usize, filter: &GpuFilter, min_allowed: usize,
                               stages: &[u32], fallback: c_int) -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = elements.len();
        if nq == 0 { return Ok(Vec::new()); }
        assert_eq!(filter.len(), self.num_elements());
        let stream = Stream::new(self.device())?;
        let q = self.upload_queries(elements, &stream)?;
        let out = DeviceResults::new(nq, num_neighbors, self.device())?;
        check(unsafe { granne_hip_search_postfiltered_batch_device(self.handle, q.ptr as *const c_void, nq as u32,
            num_neighbors as u32, min_allowed as u32, stages.as_ptr(), stages.len() as u32, fallback,
            filter.words.ptr as *const u32, 0, 0, out.ids.ptr, out.dists.ptr, out.counts.ptr, std::ptr::null_mut(),
            std::ptr::null_mut(), stream.raw) })?;
        out.to_host(nq, &stream)
    }
    /// `granne_hip_exact_range_device`: every element within `radii[i]` of query i, exact by construction -- the nearest
    /// `cap` (up to `GRANNE_HIP_RANGE_CAP_MAX`) of them ascending by (distance, id), and `totals[i]`, the exact number
    /// within the radius also beyond `cap`. `filter`: `None` for all rows, else the rows one bitmap allows. The call
    /// waits on its stream once.
    pub fn exact_range(&self, elements: &[E::Vector], radii: &[f32], cap: usize, filter: Option<&GpuFilter>)
                       -> std::io::Result<(Vec<Vec<(usize, f32)>>, Vec<u32>)> {
        let nq = elements.len();
        assert_eq!(nq, radii.len());
        if nq == 0 { return Ok((Vec::new(), Vec::new())); }
        if let Some(f) = filter { assert_eq!(f.len(), self.num_elements()); }
        let stream = Stream::new(self.device())?;
        let q = self.upload_queries(elements, &stream)?;
        let r = DeviceBuffer::<f32>::new(nq, self.device())?;
        r.copy_from(radii, &stream)?;
        let out = DeviceResults::new(nq, cap, self.device())?;
        let totals = DeviceBuffer::<u32>::new(nq, self.device())?;
        check(unsafe { granne_hip_exact_range_device(self.handle, q.ptr as *const c_void, nq as u32, r.ptr as *const f32,
            cap as u32, filter.map_or(std::ptr::null(), |f| f.words.ptr as *const u32), 0, out.ids.ptr, out.dists.ptr,
            out.counts.ptr, totals.ptr, std::ptr::null_mut(), stream.raw) })?;
        let mut t = vec![0u32; nq];
        totals.copy_to(&mut t, &stream)?;
        Ok((out.to_host(nq, &stream)?, t))
    }
    /// `granne_hip_search_range_batch_device`: the elements within `radii[i]` of query i by the ordinary search with
    /// lists of `stages[s]` entries, cut at the radius. A query is answered by the first stage whose list holds an entry
    /// beyond the radius (or whose walk ran out of graph); what no stage finishes gets the exact scan
    /// (`GRANNE_HIP_RG_FALLBACK_EXACT`) or its short answer (`_SHORT`). Returns the answers and, per query, how many
    /// entries lay within the radius (`found`). The call waits on its stream once per stage it goes beyond.
    pub fn search_range(&self, elements: &[E::Vector], radii: &[f32], cap: usize, stages: &[u32], fallback: c_int)
                        -> std::io::Result<(Vec<Vec<(usize, f32)>>, Vec<u32>)> {
        let nq = elements.len();
        assert_eq!(nq, radii.len());
        if nq == 0 { return Ok((Vec::new(), Vec::new())); }
        let stream = Stream::new(self.device())?;
        let q = self.upload_queries(elements, &stream)?;
        let r = DeviceBuffer::<f32>::new(nq, self.device())?;
        r.copy_from(radii, &stream)?;
        let out = DeviceResults::new(nq, cap, self.device())?;
        let found = DeviceBuffer::<u32>::new(nq, self.device())?;
        check(unsafe { granne_hip_search_range_batch_device(self.handle, q.ptr as *const c_void, nq as u32,
            r.ptr as *const f32, cap as u32, stages.as_ptr(), stages.len() as u32, fallback, 0, out.ids.ptr, out.dists.ptr,
            out.counts.ptr, found.ptr, std::ptr::null_mut(), std::ptr::null_mut(), stream.raw) })?;
        let mut f = vec![0u32; nq];
        found.copy_to(&mut f, &stream)?;
        Ok((out.to_host(nq, &stream)?, f))
    }
    /// Rows of the element set (at least `len()`): what `exact_topk` and `exact_topk_filtered` scan.
    pub fn num_elements(&self) -> usize { unsafe { granne_hip_index_num_elements(self.handle) as usize } }
    /// `granne_hip_search_refined_batch`: walk `self` (say, int8 rows and their graph), give the walk's `refine_from` best
    /// candidates their distances under `refine`'s rows (say, the f32 rows of the same elements; a handle made with no
    /// layers is enough) and keep the `num_neighbors` best by (distance, id). `walk_elements[i]` and `refine_elements[i]`
    /// are query i prepared for each index. `1 <= refine_from <= min(max_search, 1024)`.
    pub fn refined<R: GpuElements>(&self, refine: &GpuGranne<R>, walk_elements: &[E::Vector], refine_elements: &[R::Vector],
                                   max_search: usize, refine_from: usize, num_neighbors: usize)
                                   -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = walk_elements.len();
        assert_eq!(nq, refine_elements.len());
        let (mut qw, mut qr) = (Vec::new(), Vec::new());
        for e in walk_elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut qw, e); }
        for e in refine_elements { assert_eq!(R::query_len(e), refine.dim); R::append_query(&mut qr, e); }
        let (mut ids, mut ds) = (vec![0u64; nq * num_neighbors], vec![0f32; nq * num_neighbors]);
        let mut counts = vec![0u32; nq];
        check(unsafe { granne_hip_search_refined_batch(self.handle, refine.handle, qw.as_ptr() as *const c_void,
            qr.as_ptr() as *const c_void, nq as u32, max_search as u32, refine_from as u32, num_neighbors as u32,
            ids.as_mut_ptr(), ds.as_mut_ptr(), counts.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut()) })?;
        Ok((0..nq).map(|i| (0..counts[i] as usize)
            .map(|j| (ids[i * num_neighbors + j] as usize, ds[i * num_neighbors + j])).collect()).collect())
    }
    /// `granne_hip_search_refined_sum_embeddings_batch`: `refined` with a SumEmbeddings container as the re-ranking side.
    /// Every candidate's f32 vector is made from its terms inside the re-rank kernel, so no dense f32 rows are held;
    /// the distances are the container's own. `refine_queries`: `nq x se.dim()` prepared (normalised) floats.
    pub fn refined_sum_embeddings(&self, se: &GpuSumEmbeddings, walk_elements: &[E::Vector], refine_queries: &[f32],
                                  max_search: usize, refine_from: usize, num_neighbors: usize)
                                  -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = walk_elements.len();
        assert_eq!(nq * se.dim(), refine_queries.len());
        let mut qw = Vec::new();
        for e in walk_elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut qw, e); }
        let (mut ids, mut ds) = (vec![0u64; nq * num_neighbors], vec![0f32; nq * num_neighbors]);
        let mut counts = vec![0u32; nq];
        check(unsafe { granne_hip_search_refined_sum_embeddings_batch(self.handle, se.handle, qw.as_ptr() as *const c_void,
            refine_queries.as_ptr() as *const c_void, nq as u32, max_search as u32, refine_from as u32, num_neighbors as u32,
            ids.as_mut_ptr(), ds.as_mut_ptr(), counts.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut()) })?;
        Ok((0..nq).map(|i| (0..counts[i] as usize)
            .map(|j| (ids[i * num_neighbors + j] as usize, ds[i * num_neighbors + j])).collect()).collect())
    }
    // ---- the device-resident entries, safe: buffers and streams are owned types (below), a batch in flight BORROWS its
    // buffers until it is ended, so the compiler keeps them alive and unaliased for exactly as long as the GPU uses them
    /// Queries of one batch in HBM (`Vector::from` applied on the host: `E::append_query`).
    pub fn upload_queries(&self, elements: &[E::Vector], stream: &Stream) -> std::io::Result<DeviceBuffer<u8>> {
        let mut q = Vec::new();
        for e in elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut q, e); }
        let bytes = unsafe { std::slice::from_raw_parts(q.as_ptr() as *const u8, q.len() * std::mem::size_of_val(&q[0])) };
        let buf = DeviceBuffer::<u8>::new(bytes.len(), self.device())?;
        buf.copy_from(bytes, stream)?;
        stream.synchronize()?; // (`q` is dropped at the end of this function: the copy has to be over)
        Ok(buf)
    }
    pub fn device(&self) -> i32 { unsafe { granne_hip_index_device(self.handle) } }
    /// `granne_hip_search_batch_device`: one batch, one launch, ordered on `stream`.
    pub fn search_batch_device(&self, queries: &DeviceBuffer<u8>, nq: usize, max_search: usize, out: &mut DeviceResults,
                               stream: &Stream) -> std::io::Result<()> {
        out.fits(nq)?;
        check(unsafe { granne_hip_search_batch_device(self.handle, queries.ptr as *const c_void, nq as u32, max_search as u32,
            out.k as u32, out.ids.ptr, out.dists.ptr, out.counts.ptr, std::ptr::null_mut(), std::ptr::null_mut(), stream.raw) })
    }
    /// `granne_hip_search_filtered_batch_device`: the batch among the ids `filter` allows (one bitmap for all queries),
    /// ordered on `stream`. `max_expand` > 0 caps a walk's bottom-layer expansions. A result holds fewer than k ids when
    /// the walk met fewer allowed ones. F16 and compact SumEmbeddings handles are refused.
    pub fn search_filtered_batch_device(&self, queries: &DeviceBuffer<u8>, nq: usize, max_search: usize, filter: &GpuFilter,
                                        max_expand: u64, out: &mut DeviceResults, stream: &Stream) -> std::io::Result<()> {
        out.fits(nq)?;
        assert_eq!(filter.len(), self.len());
        check(unsafe { granne_hip_search_filtered_batch_device(self.handle, queries.ptr as *const c_void, nq as u32,
            max_search as u32, out.k as u32, filter.words.ptr as *const u32, 0, max_expand, out.ids.ptr, out.dists.ptr,
            out.counts.ptr, std::ptr::null_mut(), std::ptr::null_mut(), stream.raw) })
    }
    /// `Granne::search` among the ids `filter` allows: `[(id, distance)]` ascending by (distance, id).
    pub fn search_filtered(&self, element: &E::Vector, filter: &GpuFilter, max_search: usize, num_neighbors: usize,
                           max_expand: u64) -> std::io::Result<Vec<(usize, f32)>> {
        let stream = Stream::new(self.device())?;
        let q = self.upload_queries(std::slice::from_ref(element), &stream)?;
        let mut out = DeviceResults::new(1, num_neighbors, self.device())?;
        self.search_filtered_batch_device(&q, 1, max_search, filter, max_expand, &mut out, &stream)?;
        Ok(out.to_host(1, &stream)?.remove(0))
    }
    /// `granne_hip_search_batches_device`: several batches of `nq` queries in ONE launch (the 5.7 M f32 / 21.8 M int8
    /// queries/s path of DESIGN.md 5): walks of later batches take the places of finished ones inside the launch.
    pub fn search_batches_device(&self, queries: &[&DeviceBuffer<u8>], nq: usize, max_search: usize,
                                 out: &mut [DeviceResults], stream: &Stream) -> std::io::Result<()> {
        assert_eq!(queries.len(), out.len());
        let k = out.first().map(|o| o.k).unwrap_or(0);
        for o in out.iter() { o.fits(nq)?; assert_eq!(o.k, k); }
        let q: Vec<*const c_void> = queries.iter().map(|b| b.ptr as *const c_void).collect();
        let ids: Vec<*mut u64> = out.iter().map(|o| o.ids.ptr).collect();
        let ds: Vec<*mut f32> = out.iter().map(|o| o.dists.ptr).collect();
        let cs: Vec<*mut u32> = out.iter().map(|o| o.counts.ptr).collect();
        check(unsafe { granne_hip_search_batches_device(self.handle, q.len() as u32, q.as_ptr(), nq as u32, max_search as u32,
            k as u32, ids.as_ptr(), ds.as_ptr(), cs.as_ptr(), std::ptr::null(), std::ptr::null_mut(), stream.raw) })
    }
    /// `granne_hip_search_begin_device`: the batch runs on one of the index's own streams, ordered after what `stream`
    /// holds; the returned `InFlight` borrows the queries and the results until `end` (or its drop) has made `stream`
    /// wait for the search. Up to `set_search_depth` (default 3, at most 16) batches may be in flight.
    pub fn begin<'a>(&'a self, queries: &'a DeviceBuffer<u8>, nq: usize, max_search: usize, out: &'a mut DeviceResults,
                     stream: &'a Stream) -> std::io::Result<InFlight<'a, E>> {
        out.fits(nq)?;
        let mut ticket = 0u64;
        check(unsafe { granne_hip_search_begin_device(self.handle, queries.ptr as *const c_void, nq as u32, max_search as u32,
            out.k as u32, out.ids.ptr, out.dists.ptr, out.counts.ptr, std::ptr::null_mut(), std::ptr::null_mut(), stream.raw,
            &mut ticket) })?;
        Ok(InFlight { index: self, ticket, stream, done: false, _buffers: PhantomData })
    }
    /// `GRANNE_HIP_OPT_SEARCH_DEPTH`: how many `begin`s may be outstanding (short int8 walks want 8 and
    /// `GPU_MAX_HW_QUEUES` raised before the process's first HIP call).
    pub fn set_search_depth(&mut self, depth: u64) -> std::io::Result<()> {
        check(unsafe { granne_hip_index_set_option(self.handle, GRANNE_HIP_OPT_SEARCH_DEPTH, depth) })
    }
    /// `GRANNE_HIP_OPT_INLINE_TAILS`: 100-d / 200-d f32 indexes keep, for the walker, a copy of every layer in which a
    /// node's neighbor ids are followed by the tails of those neighbors' rows (whole-line reads; +6.9 GB of HBM at
    /// 10M x 100-d). On by default; `false` frees the copy. Results do not depend on it.
    pub fn set_inline_tails(&mut self, keep: bool) -> std::io::Result<()> {
        check(unsafe { granne_hip_index_set_option(self.handle, GRANNE_HIP_OPT_INLINE_TAILS, keep as u64) })
    }
    /// `GRANNE_HIP_OPT_SEEN_MIN`: f32 launches of at least this many walks skip a revisited neighbor BEFORE its row is
    /// fetched (a cache of the ids the walk has evaluated; a miss means nothing, so results do not depend on it). Default
    /// 2048; 0 = every launch; `u32::MAX as u64` = never.
    pub fn set_seen_min(&mut self, walks: u64) -> std::io::Result<()> {
        check(unsafe { granne_hip_index_set_option(self.handle, GRANNE_HIP_OPT_SEEN_MIN, walks) })
    }
    /// `GRANNE_HIP_OPT_COALESCE`: `search` calls that are inside the library at the same moment -- a rayon `par_iter` over
    /// `search`, the reference's way to throughput -- share search launches: one caller leads, takes the waiting calls of
    /// its own `(max_search, num_neighbors)`, runs one launch over all their queries and hands every call its rows.
    /// Off by default. Results and errors are those of the calls made alone. It gains nothing for one thread, or for a
    /// caller that already batches (`search_batch`, the `_device` entries). Not while a search is running.
    pub fn set_coalesce(&mut self, on: bool) -> std::io::Result<()> {
        check(unsafe { granne_hip_index_set_option(self.handle, GRANNE_HIP_OPT_COALESCE, on as u64) })
    }
    /// `GRANNE_HIP_OPT_COALESCE_MAX` (queries per grouped launch, 1..=1024) and `GRANNE_HIP_OPT_COALESCE_WAIT_US` (how long a
    /// new leader waits for its group to fill; 0 = never, the default).
    pub fn set_coalesce_limits(&mut self, max_queries: u64, wait_us: u64) -> std::io::Result<()> {
        check(unsafe { granne_hip_index_set_option(self.handle, GRANNE_HIP_OPT_COALESCE_MAX, max_queries) })?;
        check(unsafe { granne_hip_index_set_option(self.handle, GRANNE_HIP_OPT_COALESCE_WAIT_US, wait_us) })
    }
    /// `(launches, queries)` of `GRANNE_HIP_OPT_COALESCED_LAUNCHES` / `_QUERIES`: their quotient is the mean group size.
    pub fn coalesced(&self) -> std::io::Result<(u64, u64)> {
        let (mut launches, mut queries) = (0u64, 0u64);
        check(unsafe { granne_hip_index_get_option(self.handle, GRANNE_HIP_OPT_COALESCED_LAUNCHES, &mut launches) })?;
        check(unsafe { granne_hip_index_get_option(self.handle, GRANNE_HIP_OPT_COALESCED_QUERIES, &mut queries) })?;
        Ok((launches, queries))
    }
    // ---- the Index trait's accessors (src/index/mod.rs:54-71); `impl Index for GpuGranne` below forwards to them
    pub fn len(&self) -> usize { unsafe { granne_hip_index_len(self.handle) as usize } }
    pub fn num_layers(&self) -> usize { unsafe { granne_hip_index_num_layers(self.handle) as usize } }
    pub fn layer_len(&self, layer: usize) -> usize { unsafe { granne_hip_index_layer_len(self.handle, layer as u32) as usize } }
    pub fn get_neighbors(&self, index: usize, layer: usize) -> Vec<usize> {
        let mut buf = vec![0u32; 512];
        let mut n = 0u32;
        check(unsafe { granne_hip_index_get_neighbors(self.handle, index as u64, layer as u32, buf.as_mut_ptr(),
            buf.len() as u32, &mut n) }).expect("granne_hip_index_get_neighbors");
        buf[..n as usize].iter().map(|&i| i as usize).collect()
    }
    /// `Granne::reorder` (src/index/reorder.rs:59-85): `permutation[i] == j` means the element with idx `j`
    /// has been moved to idx `i`.
    pub fn reorder(&mut self, _show_progress: bool) -> Vec<usize> {
        let mut order = vec![0u64; self.len()];
        check(unsafe { granne_hip_index_reorder(self.handle, order.as_mut_ptr()) }).expect("granne_hip_index_reorder");
        order.into_iter().map(|i| i as usize).collect()
    }
    pub fn reorder_by_keys(&mut self, keys: &[u64], _show_progress: bool) -> Vec<usize> {
        assert_eq!(self.len(), keys.len()); // reorder.rs:91
        let mut order = vec![0u64; self.len()];
        check(unsafe { granne_hip_index_reorder_by_keys(self.handle, keys.as_ptr(), order.as_mut_ptr()) })
            .expect("granne_hip_index_reorder_by_keys");
        order.into_iter().map(|i| i as usize).collect()
    }
    /// `ElementContainer::dists(&self, element, indices)` (src/elements/mod.rs:35-39)
    pub fn dists(&self, element: &E::Vector, indices: &[usize]) -> Vec<f32> {
        let ids: Vec<u32> = indices.iter().map(|&i| i as u32).collect();
        let qidx = vec![0u32; ids.len()];
        let mut out = vec![0f32; ids.len()];
        check(unsafe { granne_hip_dist_pairs(self.handle, E::query_scalars(element), 1, qidx.as_ptr(), ids.as_ptr(),
            ids.len() as u64, out.as_mut_ptr()) }).expect("granne_hip_dist_pairs");
        out
    }
}
impl<E: GpuElements> Drop for GpuGranne<E> { fn drop(&mut self) { unsafe { granne_hip_index_destroy(self.handle) } } }

/// `embeddings::SumEmbeddings` (src/elements/embeddings/mod.rs:41-216) as the library holds it: the table and the elements'
/// term lists (CSR). The re-ranking side of `GpuGranne::refined_sum_embeddings`; `rows` gives its elements as prepared
/// rows of a dense element type, which is what the index to walk is built from.
pub struct GpuSumEmbeddings { handle: *mut granne_hip_sum_embeddings }
unsafe impl Send for GpuSumEmbeddings {}
impl GpuSumEmbeddings {
    /// `table`: `n_embeddings x dim` floats, not normalised; `offsets`: `n + 1` positions in `terms`, the first 0.
    pub fn new(table: &[f32], dim: usize, offsets: &[u64], terms: &[u32], device: i32) -> std::io::Result<Self> {
        assert!(dim > 0 && table.len() % dim == 0 && !offsets.is_empty());
        let mut handle = std::ptr::null_mut();
        check(unsafe { granne_hip_sum_embeddings_create(&mut handle, table.as_ptr(), (table.len() / dim) as u64, dim as u32,
            offsets.as_ptr(), terms.as_ptr(), (offsets.len() - 1) as u64, device) })?;
        Ok(Self { handle })
    }
    pub fn len(&self) -> usize { unsafe { granne_hip_sum_embeddings_len(self.handle) as usize } }
    pub fn dim(&self) -> usize { unsafe { granne_hip_sum_embeddings_dim(self.handle) as usize } }
    /// `granne_hip_sum_embeddings_rows` for `GRANNE_HIP_I8`: elements `first .. first + count` normalised and quantised,
    /// `count x dim` bytes -- the rows of the int8 index that `refined_sum_embeddings` walks.
    pub fn rows_i8(&self, first: usize, count: usize) -> std::io::Result<Vec<i8>> {
        let mut out = vec![0i8; count * self.dim()];
        check(unsafe { granne_hip_sum_embeddings_rows(self.handle, first as u64, count as u64, GRANNE_HIP_I8,
            out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }
}
impl Drop for GpuSumEmbeddings { fn drop(&mut self) { unsafe { granne_hip_sum_embeddings_destroy(self.handle) } } }

/// The reference's `Index` trait (src/index/mod.rs:54-71): code that is generic over `Index` takes a `GpuGranne`.
impl<E: GpuElements> Index for GpuGranne<E> {
    fn len(self: &Self) -> usize { GpuGranne::len(self) }
    fn num_layers(self: &Self) -> usize { GpuGranne::num_layers(self) }
    fn layer_len(self: &Self, layer: usize) -> usize { GpuGranne::layer_len(self, layer) }
    fn get_neighbors(self: &Self, index: usize, layer: usize) -> Vec<usize> { GpuGranne::get_neighbors(self, index, layer) }
    /// `io::write_index` (src/index/io.rs:11-70) of the layers in HBM: the library downloads and encodes them
    /// (granne's compressed format), the bytes go to `buffer` as they are.
    fn write_index<B: std::io::Write + std::io::Seek>(self: &Self, buffer: &mut B) -> std::io::Result<()> {
        let mut bytes: *mut c_void = std::ptr::null_mut();
        let mut len = 0u64;
        check(unsafe { granne_hip_index_encode(self.handle, &mut bytes, &mut len) })?;
        let res = buffer.write_all(unsafe { std::slice::from_raw_parts(bytes as *const u8, len as usize) });
        unsafe { granne_hip_bytes_free(bytes) };
        res
    }
}

/// A batch begun with `GpuGranne::begin` and not yet ended. Ending (explicitly, or by drop) makes the caller's stream
/// wait for the search; the borrow of the query and result buffers ends with this value.
pub struct InFlight<'a, E: GpuElements> {
    index: &'a GpuGranne<E>, ticket: u64, stream: &'a Stream, done: bool,
    _buffers: PhantomData<(&'a DeviceBuffer<u8>, &'a mut DeviceResults)>,
}
impl<'a, E: GpuElements> InFlight<'a, E> {
    pub fn end(mut self) -> std::io::Result<()> { self.finish() }
    fn finish(&mut self) -> std::io::Result<()> {
        if self.done { return Ok(()); }
        self.done = true;
        check(unsafe { granne_hip_search_end_device(self.index.handle, self.ticket, self.stream.raw) })
    }
}
impl<'a, E: GpuElements> Drop for InFlight<'a, E> { fn drop(&mut self) { let _ = self.finish(); } }

/// `hipStream_t`, created and destroyed through the library (a host with HIP bindings of its own wraps its stream with
/// `Stream::borrowed` instead).
pub struct Stream { raw: *mut c_void, device: i32, owned: bool }
unsafe impl Send for Stream {}
impl Stream {
    pub fn new(device: i32) -> std::io::Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { granne_hip_stream_create(&mut raw, device) })?;
        Ok(Self { raw, device, owned: true })
    }
    /// # Safety: `raw` is a live hipStream_t of `device` for as long as the value exists.
    pub unsafe fn borrowed(raw: *mut c_void, device: i32) -> Self { Self { raw, device, owned: false } }
    pub fn synchronize(&self) -> std::io::Result<()> { check(unsafe { granne_hip_stream_synchronize(self.raw, self.device) }) }
}
impl Drop for Stream {
    fn drop(&mut self) { if self.owned { unsafe { granne_hip_stream_synchronize(self.raw, self.device); granne_hip_stream_destroy(self.raw, self.device); } } }
}

/// `len` values of `T` in the HBM of one device.
pub struct DeviceBuffer<T: Copy> { ptr: *mut T, len: usize, device: i32 }
unsafe impl<T: Copy> Send for DeviceBuffer<T> {}
impl<T: Copy> DeviceBuffer<T> {
    pub fn new(len: usize, device: i32) -> std::io::Result<Self> {
        let mut p = std::ptr::null_mut();
        check(unsafe { granne_hip_device_malloc(&mut p, (len * std::mem::size_of::<T>()) as u64, device) })?;
        Ok(Self { ptr: p as *mut T, len, device })
    }
    pub fn len(&self) -> usize { self.len }
    /// host -> device, ordered on `stream`; `src` must stay alive until the stream has passed the copy (synchronize, or
    /// keep it in a structure that outlives the work: pageable memory is staged by the runtime before the call returns)
    pub fn copy_from(&self, src: &[T], stream: &Stream) -> std::io::Result<()> {
        assert!(src.len() <= self.len);
        check(unsafe { granne_hip_copy_to_device(self.ptr as *mut c_void, src.as_ptr() as *const c_void,
            (src.len() * std::mem::size_of::<T>()) as u64, self.device, stream.raw) })
    }
    /// device -> host; returns after `stream` has been waited for (the data is in `dst`)
    pub fn copy_to(&self, dst: &mut [T], stream: &Stream) -> std::io::Result<()> {
        assert!(dst.len() <= self.len);
        check(unsafe { granne_hip_copy_to_host(dst.as_mut_ptr() as *mut c_void, self.ptr as *const c_void,
            (dst.len() * std::mem::size_of::<T>()) as u64, self.device, stream.raw) })?;
        stream.synchronize()
    }
}
impl<T: Copy> Drop for DeviceBuffer<T> { fn drop(&mut self) { unsafe { granne_hip_device_free(self.ptr as *mut c_void, self.device); } } }

/// An id bitmap in HBM for `search_filtered`: bit (id & 31) of u32 word (id >> 5) over the ids 0..n-1.
pub struct GpuFilter { words: DeviceBuffer<u32>, n: usize }
impl GpuFilter {
    fn empty(n: usize, device: i32) -> std::io::Result<Self> {
        let mut w = 0u64;
        check(unsafe { granne_hip_filter_words(n as u64, &mut w) })?;
        Ok(Self { words: DeviceBuffer::new(w as usize, device)?, n })
    }
    /// The bits of `ids` set (duplicates are harmless); returns the filter and how many ids were >= n (left out).
    pub fn from_ids(ids: &[u64], n: usize, device: i32) -> std::io::Result<(Self, u32)> {
        let (f, stream) = (Self::empty(n, device)?, Stream::new(device)?);
        let d_ids = DeviceBuffer::<u64>::new(ids.len().max(1), device)?;
        d_ids.copy_from(ids, &stream)?;
        let d_bad = DeviceBuffer::<u32>::new(1, device)?;
        d_bad.copy_from(&[0u32], &stream)?;
        check(unsafe { granne_hip_filter_from_ids_device(d_ids.ptr as *const u64, ids.len() as u64, n as u64, f.words.ptr,
            d_bad.ptr, device, stream.raw) })?;
        let mut bad = [0u32];
        d_bad.copy_to(&mut bad, &stream)?;
        Ok((f, bad[0]))
    }
    /// One entry per id, `true` = allowed.
    pub fn from_mask(mask: &[bool], device: i32) -> std::io::Result<Self> {
        let (f, stream) = (Self::empty(mask.len(), device)?, Stream::new(device)?);
        let bytes: Vec<u8> = mask.iter().map(|&b| b as u8).collect();
        let d_mask = DeviceBuffer::<u8>::new(bytes.len().max(1), device)?;
        d_mask.copy_from(&bytes, &stream)?;
        check(unsafe { granne_hip_filter_from_mask_device(d_mask.ptr as *const u8, mask.len() as u64, f.words.ptr, device, stream.raw) })?;
        stream.synchronize()?;
        Ok(f)
    }
    /// Number of allowed ids.
    pub fn count(&self) -> std::io::Result<u64> {
        let stream = Stream::new(self.words.device)?;
        let d_out = DeviceBuffer::<u64>::new(1, self.words.device)?;
        check(unsafe { granne_hip_filter_count_device(self.words.ptr as *const u32, self.n as u64, d_out.ptr, self.words.device, stream.raw) })?;
        let mut out = [0u64];
        d_out.copy_to(&mut out, &stream)?;
        Ok(out[0])
    }
    /// The allowed ids, ascending: what `from_ids` would take back.
    pub fn ids(&self) -> std::io::Result<Vec<u64>> {
        let stream = Stream::new(self.words.device)?;
        let d_ids = DeviceBuffer::<u64>::new(self.n.max(1), self.words.device)?;
        let d_count = DeviceBuffer::<u64>::new(1, self.words.device)?;
        check(unsafe { granne_hip_filter_to_ids_device(self.words.ptr as *const u32, self.n as u64, d_ids.ptr, d_count.ptr,
            self.words.device, stream.raw) })?;
        let mut m = [0u64];
        d_count.copy_to(&mut m, &stream)?;
        let mut out = vec![0u64; self.n];
        d_ids.copy_to(&mut out, &stream)?;
        out.truncate(m[0] as usize);
        Ok(out)
    }
    pub fn len(&self) -> usize { self.n }
}

/// The results of one batch in HBM: `[nq][k]` ids and distances, `[nq]` counts.
pub struct DeviceResults { pub ids: DeviceBuffer<u64>, pub dists: DeviceBuffer<f32>, pub counts: DeviceBuffer<u32>, nq: usize, k: usize }
impl DeviceResults {
    pub fn new(nq: usize, k: usize, device: i32) -> std::io::Result<Self> {
        Ok(Self { ids: DeviceBuffer::new(nq * k, device)?, dists: DeviceBuffer::new(nq * k, device)?,
                  counts: DeviceBuffer::new(nq, device)?, nq, k })
    }
    fn fits(&self, nq: usize) -> std::io::Result<()> {
        if nq <= self.nq { Ok(()) } else { Err(std::io::Error::new(std::io::ErrorKind::InvalidInput, "result buffers are smaller than the batch")) }
    }
    /// `Vec<Vec<(usize, f32)>>` as `Granne::search` returns it, one per query (waits for `stream`)
    pub fn to_host(&self, nq: usize, stream: &Stream) -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let (mut ids, mut ds, mut cs) = (vec![0u64; nq * self.k], vec![0f32; nq * self.k], vec![0u32; nq]);
        self.ids.copy_to(&mut ids, stream)?;
        self.dists.copy_to(&mut ds, stream)?;
        self.counts.copy_to(&mut cs, stream)?;
        Ok((0..nq).map(|i| (0..cs[i] as usize).map(|j| (ids[i * self.k + j] as usize, ds[i * self.k + j])).collect()).collect())
    }
}

pub type GpuAngularGranne<'a> = GpuGranne<angular::Vectors<'a>>;
pub type GpuAngularIntGranne<'a> = GpuGranne<angular_int::Vectors<'a>>;

/// `GranneBuilder` on the GPU: the same layer pyramid and per-element work, a deterministic batched
/// insertion schedule instead of rayon + per-node locks.
pub struct GpuGranneBuilder<E: GpuElements> { handle: *mut granne_hip_builder, _e: PhantomData<E> }
unsafe impl<E: GpuElements> Send for GpuGranneBuilder<E> {}

/// `BuildConfig` (src/index/mod.rs:198-283) for the GPU builder: the same builder-style methods, the same defaults.
/// `BuildConfig`'s own fields are private to `index` and it has no getters (mod.rs:199-214), so a back end outside
/// that module cannot read one; inside the granne crate a maintainer adds `pub(crate)` getters and
/// `impl From<BuildConfig> for GpuBuildConfig`, and every `GpuBuildConfig` below can be spelled `BuildConfig`.
#[derive(Clone, Debug)]
pub struct GpuBuildConfig {
    layer_multiplier: f32,
    expected_num_elements: Option<usize>,
    num_neighbors: usize,
    max_search: usize,
    reinsert_elements: bool,
    show_progress: bool,
}
impl Default for GpuBuildConfig {
    /// mod.rs:217-231
    fn default() -> Self {
        Self { layer_multiplier: 15.0, expected_num_elements: None, num_neighbors: 30, max_search: 200,
               reinsert_elements: true, show_progress: false }
    }
}
impl GpuBuildConfig {
    pub fn new() -> Self { Self::default() }
    pub fn layer_multiplier(mut self, layer_multiplier: f32) -> Self { self.layer_multiplier = layer_multiplier; self }
    pub fn expected_num_elements(mut self, n: usize) -> Self { self.expected_num_elements = Some(n); self }
    pub fn num_neighbors(mut self, num_neighbors: usize) -> Self { self.num_neighbors = num_neighbors; self }
    pub fn max_search(mut self, max_search: usize) -> Self { self.max_search = max_search; self }
    pub fn reinsert_elements(mut self, yes: bool) -> Self { self.reinsert_elements = yes; self }
    pub fn show_progress(mut self, yes: bool) -> Self { self.show_progress = yes; self }
}

fn to_c(config: &GpuBuildConfig) -> granne_hip_build_config {
    // the batch schedule (batch_max, batch_div) keeps the library's defaults
    let mut c = std::mem::MaybeUninit::<granne_hip_build_config>::uninit();
    unsafe { granne_hip_build_config_default(c.as_mut_ptr()) };
    let mut c = unsafe { c.assume_init() };
    c.layer_multiplier = config.layer_multiplier;
    c.expected_num_elements = config.expected_num_elements.unwrap_or(0) as u64;
    c.num_neighbors = config.num_neighbors as u32;
    c.max_search = config.max_search as u32;
    c.reinsert_elements = config.reinsert_elements as c_int;
    c.show_progress = config.show_progress as c_int;
    c
}

impl<E: GpuElements> GpuGranneBuilder<E> {
    /// `GranneBuilder::new(config, elements)` (mod.rs:419-428)
    pub fn new(config: GpuBuildConfig, elements: &E, device: i32) -> std::io::Result<Self> {
        let c = to_c(&config);
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_builder_create(&mut h, &c, elements.scalars(), elements.n() as u64,
            elements.width() as u32, E::DTYPE, device) })?;
        Ok(Self { handle: h, _e: PhantomData })
    }
    /// `GranneBuilder::from_bytes(config, buffer, elements)` (mod.rs:430-461): continue from a written index
    pub fn from_bytes(config: GpuBuildConfig, buffer: &[u8], elements: &E, device: i32) -> std::io::Result<Self> {
        let b = Self::new(config, elements, device)?;
        check(unsafe { granne_hip_builder_load_index(b.handle, buffer.as_ptr() as *const c_void, buffer.len() as u64) })?;
        Ok(b)
    }
    /// `Builder::push` for prepared rows (mod.rs:303-315, 527-531)
    pub fn extend(&mut self, elements: &E) -> std::io::Result<()> {
        check(unsafe { granne_hip_builder_append(self.handle, elements.scalars(), elements.n() as u64) })
    }
    pub fn build(&mut self) { check(unsafe { granne_hip_builder_build(self.handle, GRANNE_HIP_BUILD_ALL) }).expect("build") }
    pub fn build_partial(&mut self, num_elements: usize) {
        check(unsafe { granne_hip_builder_build(self.handle, num_elements as u64) }).expect("build_partial") // 0: no-op, mod.rs:375
    }
    pub fn len(&self) -> usize { unsafe { granne_hip_builder_len(self.handle) as usize } }
    pub fn num_layers(&self) -> usize { unsafe { granne_hip_builder_num_layers(self.handle) as usize } }
    pub fn layer_len(&self, layer: usize) -> usize { unsafe { granne_hip_builder_layer_len(self.handle, layer as u32) as usize } }
    /// layer `layer` as a row-major [layer_len][num_neighbors] u32 matrix, UNUSED padded (host copy)
    pub fn layer_rows(&self, layer: usize, num_neighbors: usize) -> Vec<u32> {
        let mut rows = vec![0u32; self.layer_len(layer) * num_neighbors];
        check(unsafe { granne_hip_builder_get_layer(self.handle, layer as u32, rows.as_mut_ptr()) }).expect("get_layer");
        rows
    }
    /// `GranneBuilder::get_index()` (mod.rs:483-488): a searchable index over the builder's current layers
    pub fn get_index(&self) -> GpuGranne<E> {
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_builder_get_index(self.handle, &mut h) }).expect("get_index");
        GpuGranne::wrap(h)
    }
}
impl<E: GpuElements> Drop for GpuGranneBuilder<E> { fn drop(&mut self) { unsafe { granne_hip_builder_destroy(self.handle) } } }

/// `RwGranneBuilder` (src/index/rw/mod.rs:15-224) on the GPU: inserts and searches on one live graph. Methods take `&self`
/// as the reference's do; the library serialises inserts against searches with a reader-writer lock held per call
/// (coarser than the reference's per-node locks: a search sees the graph after a whole number of insert calls). Inserts
/// follow the deterministic batched schedule of the GPU builder. Without a previous layer `search` returns nothing, as
/// the reference's does (rw/mod.rs:198-206).
pub struct GpuRwGranneBuilder<E: GpuElements> { handle: *mut granne_hip_rw_builder, dim: usize, _e: PhantomData<E> }
unsafe impl<E: GpuElements> Send for GpuRwGranneBuilder<E> {}
unsafe impl<E: GpuElements> Sync for GpuRwGranneBuilder<E> {}

impl<E: GpuElements> GpuRwGranneBuilder<E> {
    /// `RwGranneBuilder::new(builder, max_elements, _)` (rw/mod.rs:32-61): consumes the builder. `dim`: the width of
    /// the builder's elements (a builder without elements has none of its own).
    pub fn new(builder: GpuGranneBuilder<E>, max_elements: usize, dim: usize) -> std::io::Result<Self> {
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_rw_builder_create(&mut h, builder.handle, max_elements as u64) })?;
        std::mem::forget(builder); // the handle owns it now
        Ok(Self { handle: h, dim, _e: PhantomData })
    }
    /// `insert` (rw/mod.rs:99-101)
    pub fn insert(&self, element: &E::Vector) -> Option<usize> {
        assert_eq!(E::query_len(element), self.dim);
        let (mut id, mut count) = (0u64, 0u64);
        check(unsafe { granne_hip_rw_builder_insert_batch(self.handle, E::query_scalars(element), 1, &mut id, &mut count) })
            .expect("insert");
        if count == 1 { Some(id as usize) } else { None }
    }
    /// `insert_batch` (rw/mod.rs:103-182): the ids of the elements that found a place
    pub fn insert_batch(&self, elements: &[E::Vector]) -> Vec<usize> {
        let mut rows = Vec::new();
        for e in elements {
            assert_eq!(E::query_len(e), self.dim);
            E::append_query(&mut rows, e);
        }
        let mut ids = vec![0u64; elements.len()];
        let mut count = 0u64;
        check(unsafe { granne_hip_rw_builder_insert_batch(self.handle, rows.as_ptr() as *const c_void, elements.len() as u64,
            ids.as_mut_ptr(), &mut count) }).expect("insert_batch");
        ids[..count as usize].iter().map(|&i| i as usize).collect()
    }
    /// `search` (rw/mod.rs:184-207)
    pub fn search(&self, element: &E::Vector, max_search: usize, num_neighbors: usize) -> Vec<(usize, f32)> {
        assert_eq!(E::query_len(element), self.dim);
        let mut ids = vec![0u64; num_neighbors];
        let mut dists = vec![0f32; num_neighbors];
        let mut count = 0u32;
        check(unsafe { granne_hip_rw_builder_search(self.handle, E::query_scalars(element), max_search as u32,
            num_neighbors as u32, ids.as_mut_ptr(), dists.as_mut_ptr(), &mut count) }).expect("search");
        (0..count as usize).map(|i| (ids[i] as usize, dists[i])).collect()
    }
    pub fn len(&self) -> usize { unsafe { granne_hip_rw_builder_len(self.handle) as usize } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }
    /// `save_index_and_elements_to_disk` (rw/mod.rs:63-68)
    pub fn save_index_and_elements_to_disk(&self, index_path: &str, elements_path: &str) -> std::io::Result<()> {
        let ip = std::ffi::CString::new(index_path).map_err(|e| std::io::Error::new(std::io::ErrorKind::InvalidInput, e))?;
        let ep = std::ffi::CString::new(elements_path).map_err(|e| std::io::Error::new(std::io::ErrorKind::InvalidInput, e))?;
        check(unsafe { granne_hip_rw_builder_save(self.handle, ip.as_ptr(), ep.as_ptr()) })
    }
    /// sub-batches of up to this many link-update ops sort them in one workgroup (0: never, 1: the default)
    pub fn set_small_ops(&self, value: u64) -> std::io::Result<()> {
        check(unsafe { granne_hip_rw_builder_set_option(self.handle, GRANNE_HIP_RW_OPT_SMALL_OPS, value) })
    }
    /// Marks the elements removed (hnswlib's markDelete): `search` never returns them again; they stay in the graph, are
    /// traversed and may be linked to, and their slots are not reused. Returns (newly removed, removed already -- repeats
    /// within `ids` included --, ids >= len, which are ignored).
    pub fn remove(&self, ids: &[u64]) -> std::io::Result<(u64, u64, u64)> {
        let mut c = [0u64; 3];
        check(unsafe { granne_hip_rw_builder_remove(self.handle, ids.as_ptr(), ids.len() as u64, c.as_mut_ptr()) })?;
        Ok((c[0], c[1], c[2]))
    }
    /// The inverse of `remove`: (newly restored, alive already, ids >= len).
    pub fn restore(&self, ids: &[u64]) -> std::io::Result<(u64, u64, u64)> {
        let mut c = [0u64; 3];
        check(unsafe { granne_hip_rw_builder_restore(self.handle, ids.as_ptr(), ids.len() as u64, c.as_mut_ptr()) })?;
        Ok((c[0], c[1], c[2]))
    }
    pub fn removed_count(&self) -> usize { unsafe { granne_hip_rw_builder_removed_count(self.handle) as usize } }
    /// A copy of the bitmap of the elements that are not removed, over the ids 0..len-1, on `device` (the handle's): the
    /// filter for `search_filtered` on a snapshot taken with no insert in between.
    pub fn alive_filter(&self, device: i32) -> std::io::Result<GpuFilter> {
        let n = self.len();
        let max = unsafe { granne_hip_rw_builder_max_elements(self.handle) as usize };
        let (mut f, stream) = (GpuFilter::empty(n.max(max), device)?, Stream::new(device)?); // (room for concurrent inserts)
        f.n = n;
        check(unsafe { granne_hip_rw_builder_alive(self.handle, f.words.ptr, stream.raw) })?;
        stream.synchronize()?;
        Ok(f)
    }
    /// A new, independent builder over the elements that are not removed, in ascending old-id order, its graph built
    /// afresh under this one's config; and `old_ids[new_id]`. `self` is left as it is.
    pub fn compact(&self, max_elements: usize) -> std::io::Result<(Self, Vec<u64>)> {
        let max = unsafe { granne_hip_rw_builder_max_elements(self.handle) as usize };
        let mut old = vec![0u64; self.len().max(max)];
        let (mut h, mut count) = (std::ptr::null_mut(), 0u64);
        check(unsafe { granne_hip_rw_builder_compact(self.handle, max_elements as u64, &mut h, old.as_mut_ptr(), &mut count) })?;
        old.truncate(count as usize);
        Ok((Self { handle: h, dim: self.dim, _e: PhantomData }, old))
    }
}
impl<E: GpuElements> Drop for GpuRwGranneBuilder<E> { fn drop(&mut self) { unsafe { granne_hip_rw_builder_destroy(self.handle) } } }

/// A partitioned index: shard `s` is a `GpuGranne` of its own (on the device it was created on) over the
/// elements `[offsets[s], offsets[s] + shard.len())` of the whole set -- how the reference's own shard helper
/// cuts an element file (src/elements/embeddings/parsing.rs:63-100). `search` asks every shard and merges by
/// (distance, global id); ids in the result are global.
pub struct GpuShardedGranne<E: GpuElements> { handle: *mut granne_hip_sharded, shards: Vec<GpuGranne<E>>, dim: usize }
unsafe impl<E: GpuElements> Send for GpuShardedGranne<E> {}

impl<E: GpuElements> GpuShardedGranne<E> {
    pub fn new(shards: Vec<GpuGranne<E>>, offsets: &[u64]) -> std::io::Result<Self> {
        assert_eq!(shards.len(), offsets.len());
        let hs: Vec<*mut granne_hip_index> = shards.iter().map(|s| s.handle).collect();
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_sharded_create(&mut h, hs.as_ptr(), offsets.as_ptr(), hs.len() as u32) })?;
        let dim = shards[0].dim;
        Ok(Self { handle: h, shards, dim })
    }
    /// The whole element set in, a searchable partitioned index out: `n_shards` id ranges
    /// (src/elements/embeddings/parsing.rs:72-98), each built with the GPU builder under `config` on
    /// `devices[s / ceil(n_shards / devices.len())]`. The handle owns its shards (`shards` stays empty).
    pub fn build(config: GpuBuildConfig, elements: &E, n_shards: usize, devices: &[i32]) -> std::io::Result<Self> {
        let cfg = to_c(&config);
        let mut h = std::ptr::null_mut();
        check(unsafe { granne_hip_sharded_build(&mut h, &cfg, elements.scalars(), elements.n() as u64,
            elements.width() as u32, E::DTYPE, n_shards as u32, devices.as_ptr(), devices.len() as u32) })?;
        Ok(Self { handle: h, shards: Vec::new(), dim: elements.width() })
    }
    pub fn len(&self) -> usize { unsafe { granne_hip_sharded_len(self.handle) as usize } }
    pub fn num_shards(&self) -> usize { unsafe { granne_hip_sharded_num_shards(self.handle) as usize } }
    pub fn search(&mut self, element: &E::Vector, max_search: usize, num_neighbors: usize) -> Vec<(usize, f32)> {
        self.search_batch(std::slice::from_ref(element), max_search, num_neighbors).pop().unwrap()
    }
    pub fn search_batch(&mut self, elements: &[E::Vector], max_search: usize, num_neighbors: usize) -> Vec<Vec<(usize, f32)>> {
        let nq = elements.len();
        let mut q = Vec::new();
        for e in elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut q, e); }
        let (mut ids, mut ds) = (vec![0u64; nq * num_neighbors], vec![0f32; nq * num_neighbors]);
        let mut counts = vec![0u32; nq];
        check(unsafe { granne_hip_sharded_search_batch(self.handle, q.as_ptr() as *const c_void, nq as u32,
            max_search as u32, num_neighbors as u32, ids.as_mut_ptr(), ds.as_mut_ptr(), counts.as_mut_ptr()) })
            .expect("granne_hip_sharded_search_batch");
        (0..nq).map(|i| (0..counts[i] as usize)
            .map(|j| (ids[i * num_neighbors + j] as usize, ds[i * num_neighbors + j])).collect()).collect()
    }
    /// Many batches of `nq` queries each: the library pipelines them (batch b+1 is uploaded and searched while
    /// batch b is exchanged, merged and downloaded; pinned staging inside). The caller-side loop over
    /// `search_batch`, without the bubbles.
    pub fn search_batches(&mut self, elements: &[E::Vector], nq: usize, max_search: usize, num_neighbors: usize)
        -> Vec<Vec<(usize, f32)>> {
        assert!(nq > 0 && elements.len() % nq == 0);
        let (total, nb) = (elements.len(), elements.len() / nq);
        let mut q = Vec::new();
        for e in elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut q, e); }
        let (mut ids, mut ds) = (vec![0u64; total * num_neighbors], vec![0f32; total * num_neighbors]);
        let mut counts = vec![0u32; total];
        check(unsafe { granne_hip_sharded_search_batches(self.handle, q.as_ptr() as *const c_void, nb as u32, nq as u32,
            max_search as u32, num_neighbors as u32, ids.as_mut_ptr(), ds.as_mut_ptr(), counts.as_mut_ptr()) })
            .expect("granne_hip_sharded_search_batches");
        (0..total).map(|i| (0..counts[i] as usize)
            .map(|j| (ids[i * num_neighbors + j] as usize, ds[i * num_neighbors + j])).collect()).collect()
    }
    /// `granne_hip_sharded_search_batch_device`: queries and results in the HBM of `self.device()` (shard 0's), ordered on
    /// `stream`; every shard searches the batch, the merged top-k lands in `out`.
    pub fn search_batch_device(&mut self, queries: &DeviceBuffer<u8>, nq: usize, max_search: usize, out: &mut DeviceResults,
                               stream: &Stream) -> std::io::Result<()> {
        out.fits(nq)?;
        check(unsafe { granne_hip_sharded_search_batch_device(self.handle, queries.ptr as *const c_void, nq as u32,
            max_search as u32, out.k as u32, out.ids.ptr, out.dists.ptr, out.counts.ptr, std::ptr::null_mut(), stream.raw) })
    }
    pub fn device(&self) -> i32 { unsafe { granne_hip_sharded_device(self.handle) } }
    /// `granne_hip_sharded_id_span`: the bits of a global filter, max over the shards of offset + rows.
    pub fn id_span(&self) -> usize { unsafe { granne_hip_sharded_id_span(self.handle) as usize } }
    fn upload_queries(&self, elements: &[E::Vector], stream: &Stream) -> std::io::Result<DeviceBuffer<u8>> {
        let mut q = Vec::new();
        for e in elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut q, e); }
        let buf = DeviceBuffer::<u8>::new(q.len().max(1), self.device())?;
        buf.copy_from(&q, stream)?;
        stream.synchronize()?; // (`q` is dropped at the end of this function: the copy has to be over)
        Ok(buf)
    }
    /// `granne_hip_sharded_search_filtered_batch_device`: `search_batch` among the GLOBAL ids `filter` allows (one bitmap
    /// over `id_span()` ids on `device()`): every shard walks under its slice, merged by (distance, global id).
    /// `max_expand > 0` caps each shard's walk.
    pub fn search_filtered(&mut self, elements: &[E::Vector], filter: &GpuFilter, max_search: usize, num_neighbors: usize,
                           max_expand: u64) -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = elements.len();
        if nq == 0 { return Ok(Vec::new()); }
        assert_eq!(filter.len(), self.id_span());
        let stream = Stream::new(self.device())?;
        let q = self.upload_queries(elements, &stream)?;
        let out = DeviceResults::new(nq, num_neighbors, self.device())?;
        check(unsafe { granne_hip_sharded_search_filtered_batch_device(self.handle, q.ptr as *const c_void, nq as u32,
            max_search as u32, num_neighbors as u32, filter.words.ptr as *const u32, 0, max_expand, out.ids.ptr, out.dists.ptr,
            out.counts.ptr, std::ptr::null_mut(), stream.raw) })?;
        out.to_host(nq, &stream)
    }
    /// `granne_hip_sharded_exact_topk`: the `k` nearest rows of the whole partitioned set, exact, global ids
    /// (`k <= 1024`, `num_shards() * k <= 4096`). An error when a query overflowed the selection in a shard.
    pub fn exact_topk(&mut self, elements: &[E::Vector], k: usize) -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = elements.len();
        let mut q = Vec::new();
        for e in elements { assert_eq!(E::query_len(e), self.dim); E::append_query(&mut q, e); }
        let (mut ids, mut ds) = (vec![0u64; nq * k], vec![0f32; nq * k]);
        let mut counts = vec![0u32; nq];
        check(unsafe { granne_hip_sharded_exact_topk(self.handle, q.as_ptr() as *const c_void, nq as u32, k as u32,
            ids.as_mut_ptr(), ds.as_mut_ptr(), counts.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok((0..nq).map(|i| (0..counts[i] as usize).map(|j| (ids[i * k + j] as usize, ds[i * k + j])).collect()).collect())
    }
    /// `granne_hip_sharded_exact_topk_filtered_device`: `exact_topk` among the global ids `filter` allows.
    pub fn exact_topk_filtered(&mut self, elements: &[E::Vector], k: usize, filter: &GpuFilter)
        -> std::io::Result<Vec<Vec<(usize, f32)>>> {
        let nq = elements.len();
        if nq == 0 { return Ok(Vec::new()); }
        assert_eq!(filter.len(), self.id_span());
        let stream = Stream::new(self.device())?;
        let q = self.upload_queries(elements, &stream)?;
        let out = DeviceResults::new(nq, k, self.device())?;
        check(unsafe { granne_hip_sharded_exact_topk_filtered_device(self.handle, q.ptr as *const c_void, nq as u32, k as u32,
            filter.words.ptr as *const u32, 0, out.ids.ptr, out.dists.ptr, out.counts.ptr, std::ptr::null_mut(), stream.raw) })?;
        out.to_host(nq, &stream)
    }
    /// `granne_hip_sharded_begin_device` / `_end_device`: batch b + 1 is searched while batch b is exchanged and merged.
    /// The ticket's borrow keeps the buffers alive; `ShardedInFlight::end` (or drop) orders `stream` after the merge.
    pub fn begin<'a>(&'a self, queries: &'a DeviceBuffer<u8>, nq: usize, max_search: usize, out: &'a mut DeviceResults,
                     stream: &'a Stream) -> std::io::Result<ShardedInFlight<'a, E>> {
        out.fits(nq)?;
        let mut ticket = 0u64;
        check(unsafe { granne_hip_sharded_begin_device(self.handle, queries.ptr as *const c_void, nq as u32, max_search as u32,
            out.k as u32, out.ids.ptr, out.dists.ptr, out.counts.ptr, std::ptr::null_mut(), stream.raw, &mut ticket) })?;
        Ok(ShardedInFlight { index: self, ticket, stream, done: false, _buffers: PhantomData })
    }
    /// The exchange step as ONE RCCL all-gather over the shard devices (instead of peer copies); batches in flight.
    pub fn use_rccl_all_gather(&mut self) -> std::io::Result<()> {
        check(unsafe { granne_hip_sharded_set_option(self.handle, GRANNE_HIP_SHARDED_OPT_EXCHANGE, GRANNE_HIP_SHARDED_EXCHANGE_RCCL) })
    }
    pub fn set_depth(&mut self, depth: u64) -> std::io::Result<()> {
        check(unsafe { granne_hip_sharded_set_option(self.handle, GRANNE_HIP_SHARDED_OPT_DEPTH, depth) })
    }
}
impl<E: GpuElements> Drop for GpuShardedGranne<E> {
    fn drop(&mut self) { unsafe { granne_hip_sharded_destroy(self.handle) } } // before `shards`: the handle borrows them
}
pub struct ShardedInFlight<'a, E: GpuElements> {
    index: &'a GpuShardedGranne<E>, ticket: u64, stream: &'a Stream, done: bool,
    _buffers: PhantomData<(&'a DeviceBuffer<u8>, &'a mut DeviceResults)>,
}
impl<'a, E: GpuElements> ShardedInFlight<'a, E> {
    pub fn end(mut self) -> std::io::Result<()> { self.finish() }
    fn finish(&mut self) -> std::io::Result<()> {
        if self.done { return Ok(()); }
        self.done = true;
        check(unsafe { granne_hip_sharded_end_device(self.index.handle, self.ticket, self.stream.raw) })
    }
}
impl<'a, E: GpuElements> Drop for ShardedInFlight<'a, E> { fn drop(&mut self) { let _ = self.finish(); } }
