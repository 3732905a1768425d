//! Shim that keeps the reference crate's signatures for the hot path on top of `libzebra_hip.so`.
//!
//! NOT COMPILED in this repository's build image (no Rust toolchain there); it mirrors
//! `include/zebra_hip.h` one to one and is kept mechanical on purpose.  It is a PATCH to the crate, not a parallel crate:
//! without the `standalone` feature it binds the crate's own `Embedding<N>` / `DistanceUnit` (see below).  What it replaces in emmyoh/zebra:
//! `src/distance.rs` (the metric structs' `Metric::distance`), `src/database/index/lsh.rs`
//! (`LSHIndex<N>`: new / add / search / remove / deduplicate / clear / is_empty / no_vectors / no_trees) and the
//! rayon loop of `Database::query_vectors` (`src/database/core.rs:299-303`) through `search_batch`.
#![allow(non_camel_case_types)]

use std::collections::HashMap;
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};
use std::sync::{Arc, RwLock};

use dashmap::{DashMap, DashSet};
use space::Metric;
use uuid::Uuid;

// ---- the vector type and the key type: the CRATE'S OWN (round 4) -----------------------------------------------------------
// As a patch to emmyoh/zebra this file lives INSIDE the crate (src/hip.rs, feature `hip`) and binds the
// crate's `Embedding<N>` / `DistanceUnit` -- it does not re-declare them: one type, no conversion at the boundary, and a
// `&[Embedding<N>]` handed to `insert_records` / `query_vectors` crosses the FFI as it is.  The stand-alone re-declaration
// below exists only behind the `standalone` feature, for building and testing this shim without the crate.
#[cfg(not(feature = "standalone"))]
pub use crate::{Embedding, EmbeddingPrecision}; // src/lib.rs:15-48 (as `zebra::...` when built as an external crate: `--cfg zebra_external`)
#[cfg(not(feature = "standalone"))]
pub use crate::distance::DistanceUnit; // src/distance.rs:13
// The reference's `Embedding<N>` is a plain newtype over `[f32; N]` (src/lib.rs:18) WITHOUT `#[repr(transparent)]`; the layout of a
// single-field struct is that of its field in practice, and this shim asserts what it relies on instead of assuming it:
#[cfg(not(feature = "standalone"))]
const _: () = {
    assert!(std::mem::size_of::<Embedding<4>>() == 16 && std::mem::align_of::<Embedding<4>>() == 4);
};

#[cfg(feature = "standalone")]
pub type DistanceUnit = u64; // src/distance.rs:13
#[cfg(feature = "standalone")]
pub type EmbeddingPrecision = f32; // src/lib.rs:48

/// (feature `standalone` only) `Embedding<N>` as in the reference (src/lib.rs:15-46): a newtype over `[f32; N]` with Deref / DerefMut /
/// Default / From / TryFrom.  `repr(transparent)`: a `&[Embedding<N>]` is `len * N` contiguous f32, which is what crosses the FFI.
#[cfg(feature = "standalone")]
#[repr(transparent)]
#[derive(Debug, Clone)]
pub struct Embedding<const N: usize>([EmbeddingPrecision; N]);
#[cfg(feature = "standalone")]
impl<const N: usize> std::ops::Deref for Embedding<N> {
    type Target = [EmbeddingPrecision; N];
    fn deref(&self) -> &[EmbeddingPrecision; N] {
        &self.0
    }
}
#[cfg(feature = "standalone")]
impl<const N: usize> std::ops::DerefMut for Embedding<N> {
    fn deref_mut(&mut self) -> &mut [EmbeddingPrecision; N] {
        &mut self.0
    }
}
#[cfg(feature = "standalone")]
impl<const N: usize> Default for Embedding<N> {
    fn default() -> Self {
        Self([0.0; N])
    }
}
#[cfg(feature = "standalone")]
impl<const N: usize> From<[EmbeddingPrecision; N]> for Embedding<N> {
    fn from(value: [EmbeddingPrecision; N]) -> Self {
        Self(value)
    }
}
#[cfg(feature = "standalone")]
impl<const N: usize> TryFrom<Vec<EmbeddingPrecision>> for Embedding<N> {
    type Error = Vec<EmbeddingPrecision>;
    fn try_from(value: Vec<EmbeddingPrecision>) -> Result<Self, Self::Error> {
        Ok(Self(value.try_into()?))
    }
}

pub mod ffi {
    use super::*;

    #[repr(C)]
    pub struct zh_index {
        _private: [u8; 0],
    }

    #[repr(C)]
    #[derive(Clone, Copy)]
    pub struct zh_options {
        pub dim: u32,
        pub max_node_size: u32, // LSHIndexOptions::max_node_size (lsh.rs:126)
        pub num_trees: u32,     // LSHIndexOptions::num_trees     (lsh.rs:128)
        pub seed: u64,
        pub device: i32,
        pub id_base: u64,
        pub reserve_rows: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_exact_info {
        pub batch: u64,
        pub rows_live: u64,
        pub path: u32,
        pub redone: u32,
        pub survivors: u64,
        pub launches: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_range_info {
        pub batch: u64,
        pub rows_live: u64,
        pub hits: u64,
        pub path: u32,
        pub redone: u32,
        pub candidates: u64,
        pub launches: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_join_info {
        pub rows_live: u64,
        pub pairs: u64,
        pub path: u32,
        pub redone: u32,
        pub candidates: u64,
        pub launches: u64,
        pub tiles: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_cross_info {
        pub rows_live_a: u64,
        pub rows_live_b: u64,
        pub pairs: u64,
        pub path: u32,
        pub redone: u32,
        pub candidates: u64,
        pub launches: u64,
        pub tiles: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_knn_info {
        pub rows_live: u64,
        pub lines: u64,
        pub k: u32,
        pub path: u32,
        pub redone: u32,
        pub survivors: u64,
        pub launches: u64,
        pub tiles: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_xknn_info {
        pub rows_live_a: u64,
        pub rows_live_b: u64,
        pub lines: u64,
        pub k: u32,
        pub path: u32,
        pub redone: u32,
        pub survivors: u64,
        pub launches: u64,
        pub tiles: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_knn_forest_info {
        pub rows_live: u64,
        pub lines: u64,
        pub k: u32,
        pub path: u32,
        pub trees: u32,
        pub pairs: u64,
        pub survivors: u64,
        pub redone: u32,
        pub launches: u64,
        pub tiles: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_knn_refine_info {
        pub rows_live: u64,
        pub lines: u64,
        pub in_k: u32,
        pub k: u32,
        pub listed: u64,
        pub keyed: u64,
        pub updates: u64,
        pub launches: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_knn_reverse_info {
        pub rows_live: u64,
        pub lines: u64,
        pub in_k: u32,
        pub rev_k: u32,
        pub edges: u64,
        pub kept: u64,
        pub max_degree: u64,
        pub launches: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_knn_refine_rev_info {
        pub rows_live: u64,
        pub lines: u64,
        pub in_k: u32,
        pub k: u32,
        pub listed: u64,
        pub keyed: u64,
        pub updates: u64,
        pub launches: u64,
        pub rev_k: u64,
        pub edges: u64,
        pub kept: u64,
        pub max_degree: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_knn_prune_info {
        pub rows_live: u64,
        pub lines: u64,
        pub in_k: u64,
        pub rev_k: u64,
        pub degree: u64,
        pub fill: u64,
        pub candidates: u64,
        pub kept: u64,
        pub occluded: u64,
        pub filled: u64,
        pub cut: u64,
        pub keyed: u64,
        pub launches: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_knn_descent_info {
        pub rows_live: u64,
        pub in_k: u32,
        pub rev_k: u32,
        pub k: u32,
        pub rounds: u32,
        pub rounds_run: u32,
        pub launches: u64,
        pub listed: u64,
        pub keyed: u64,
        pub lines_active: u64,
        pub updates: u64,
        pub large_lines: u64,
        pub keyed_round: [u64; 32],
        pub updates_round: [u64; 32],
        pub active_round: [u64; 32],
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_graph_info {
        pub attached: u32,
        pub g_k: u32,
        pub g_rows: u64,
        pub bytes: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_graph_search_info {
        pub queries: u64,
        pub seeds: u64,
        pub iterations: u64,
        pub expanded: u64,
        pub keyed: u64,
        pub capped: u64,
        pub launches: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_graph_filtered_info {
        pub queries: u64,
        pub seeds: u64,
        pub iterations: u64,
        pub expanded: u64,
        pub keyed: u64,
        pub capped: u64,
        pub launches: u64,
        pub rows_allowed: u64,
        pub offered: u64,
        pub returned: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_graph_steered_info {
        pub queries: u64,
        pub seeds: u64,
        pub iterations: u64,
        pub expanded: u64,
        pub keyed: u64,
        pub capped: u64,
        pub launches: u64,
        pub rows_allowed: u64,
        pub direct: u64,
        pub via_bridge: u64,
        pub bridges: u64,
        pub cand_full: u64,
        pub returned: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_graph_extend_info {
        pub rows_added: u64,
        pub rows_removed: u64,
        pub chunks: u64,
        pub seeds: u64,
        pub iterations: u64,
        pub expanded: u64,
        pub keyed: u64,
        pub capped: u64,
        pub reverse_rows: u64,
        pub reverse_offered: u64,
        pub reverse_kept: u64,
        pub launches: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_join_forest_info {
        pub rows_live: u64,
        pub trees: u32,
        pub path: u32,
        pub leaf_pairs: u64,
        pub pairs: u64,
        pub candidates: u64,
        pub launches: u64,
        pub tiles: u64,
        pub redone: u32,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_range_forest_info {
        pub batch: u64,
        pub rows_live: u64,
        pub trees: u32,
        pub probe: u32,
        pub path: u32,
        pub redone: u32,
        pub visits: u64,
        pub leaf_rows: u64,
        pub hits: u64,
        pub candidates: u64,
        pub launches: u64,
        pub tiles: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy)]
    pub struct zh_filtered_info {
        pub batch: u64,
        pub rows_live: u64,
        pub rows_allowed: u64,
        pub path: u32,
        pub redone: u32,
        pub survivors: u64,
        pub launches: u64,
        pub tiles_skipped: u64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy, Debug)]
    pub struct zh_compact_info {
        pub rows_before: u64,
        pub rows_after: u64,
        pub rows_moved: u64,
        pub bytes_moved: u64,
        pub scratch_bytes: u64,
        pub capacity_rows: u64,
        pub copy_bytes_released: u64,
        pub ms: f64,
    }

    #[repr(C)]
    #[derive(Default, Clone, Copy, Debug)]
    pub struct zh_snapshot_info {
        pub version: u32,
        pub dim: u32,
        pub max_node_size: u32,
        pub num_trees_option: u32,
        pub seed: u64,
        pub id_base: u64,
        pub stored_rows: u64,
        pub live_rows: u64,
        pub n_trees: u32,
        pub n_nodes: u32,
        pub n_planes: u32,
        pub flags: u32,
        pub n_leaf_ids: u64,
        pub file_bytes: u64,
        pub row_bytes: u64,
        pub n_sections: u32,
        pub verified: u32,
        pub ms: f64,
        pub ms_device: f64,
    }

    pub const ZH_COSINE: c_int = 0;
    pub const ZH_L2SQ: c_int = 1;
    pub const ZH_L2: c_int = 2;
    pub const ZH_CHEBYSHEV: c_int = 3;
    pub const ZH_CANBERRA: c_int = 4;
    pub const ZH_BRAY_CURTIS: c_int = 5;
    pub const ZH_MANHATTAN: c_int = 6;
    pub const ZH_L3: c_int = 7;
    pub const ZH_L4: c_int = 8;
    pub const ZH_HAMMING: c_int = 9;
    pub const ZH_MINKOWSKI: c_int = 10;
    pub const ZH_PNORM: c_int = 11;
    pub const ZH_COSINE_PARITY: c_int = 0; // distance.rs:23-25 literally
    pub const ZH_COSINE_CORRECTED: c_int = 1;

    extern "C" {
        pub fn zh_options_default(opt: *mut zh_options);
        pub fn zh_index_create(opt: *const zh_options, out: *mut *mut zh_index) -> c_int;
        pub fn zh_index_destroy(idx: *mut zh_index);
        pub fn zh_index_clear(idx: *mut zh_index) -> c_int;
        pub fn zh_index_add(idx: *mut zh_index, rows: *const f32, n: usize, out_row_ids: *mut u64) -> c_int;
        pub fn zh_index_build(idx: *mut zh_index) -> c_int;
        pub fn zh_index_remove(idx: *mut zh_index, ids: *const u64, n: usize, out_found: *mut u8, out_n_removed: *mut usize) -> c_int;
        pub fn zh_index_deduplicate(idx: *mut zh_index, out_ids: *mut u64, cap: usize, out_n_removed: *mut usize) -> c_int;
        pub fn zh_index_compact(idx: *mut zh_index, out_new_ids: *mut u64, cap: usize, info: *mut zh_compact_info) -> c_int;
        pub fn zh_index_save(idx: *mut zh_index, path: *const std::os::raw::c_char, info: *mut zh_snapshot_info) -> c_int;
        pub fn zh_index_load(path: *const std::os::raw::c_char, device: i32, reserve_rows: u64, out: *mut *mut zh_index,
                             info: *mut zh_snapshot_info) -> c_int;
        pub fn zh_index_count(idx: *const zh_index) -> u64;
        pub fn zh_index_stored_rows(idx: *const zh_index) -> u64;
        pub fn zh_index_num_trees(idx: *const zh_index) -> u32;
        pub fn zh_search_batch(idx: *mut zh_index, q: *const f32, b: usize, k: usize, metric: c_int, cosine_mode: c_int,
                               out_ids: *mut u64, out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_search_exact_batch(idx: *mut zh_index, q: *const f32, b: usize, k: usize, metric: c_int, cosine_mode: c_int,
                                     out_ids: *mut u64, out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_search_exact_batch_device(idx: *mut zh_index, d_q: *const f32, b: usize, k: usize, metric: c_int, cosine_mode: c_int,
                                            d_out_ids: *mut u64, d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_search_exact_info(idx: *const zh_index, out: *mut zh_exact_info) -> c_int;
        pub fn zh_search_exact_filtered_batch(idx: *mut zh_index, q: *const f32, b: usize, k: usize, metric: c_int, cosine_mode: c_int,
                                              filter_words: *const u32, n_bits: u64, out_ids: *mut u64, out_keys: *mut u64,
                                              out_counts: *mut u32) -> c_int;
        pub fn zh_search_exact_filtered_batch_device(idx: *mut zh_index, d_q: *const f32, b: usize, k: usize, metric: c_int, cosine_mode: c_int,
                                                     d_filter_words: *const u32, n_bits: u64, d_out_ids: *mut u64, d_out_keys: *mut u64,
                                                     d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_search_filtered_info(idx: *const zh_index, out: *mut zh_filtered_info) -> c_int;
        pub fn zh_search_range_batch(idx: *mut zh_index, q: *const f32, b: usize, max_keys: *const u64, metric: c_int, cosine_mode: c_int,
                                     capacity: u64, out_offsets: *mut u64, out_ids: *mut u64, out_keys: *mut u64, out_total: *mut u64) -> c_int;
        pub fn zh_search_range_batch_device(idx: *mut zh_index, d_q: *const f32, b: usize, d_max_keys: *const u64, metric: c_int, cosine_mode: c_int,
                                            capacity: u64, d_out_offsets: *mut u64, d_out_ids: *mut u64, d_out_keys: *mut u64, d_out_total: *mut u64,
                                            stream: *mut c_void) -> c_int;
        pub fn zh_search_range_info(idx: *const zh_index, out: *mut zh_range_info) -> c_int;
        pub fn zh_self_join(idx: *mut zh_index, max_key: u64, metric: c_int, cosine_mode: c_int, capacity: u64, out_a: *mut u64, out_b: *mut u64,
                            out_keys: *mut u64, out_total: *mut u64) -> c_int;
        pub fn zh_self_join_device(idx: *mut zh_index, max_key: u64, metric: c_int, cosine_mode: c_int, capacity: u64, d_out_a: *mut u64,
                                   d_out_b: *mut u64, d_out_keys: *mut u64, d_out_total: *mut u64, stream: *mut c_void) -> c_int;
        pub fn zh_self_join_info(idx: *const zh_index, out: *mut zh_join_info) -> c_int;
        pub fn zh_cross_join(a: *mut zh_index, b: *mut zh_index, max_key: u64, metric: c_int, cosine_mode: c_int, capacity: u64, out_a: *mut u64,
                             out_b: *mut u64, out_keys: *mut u64, out_total: *mut u64) -> c_int;
        pub fn zh_cross_join_device(a: *mut zh_index, b: *mut zh_index, max_key: u64, metric: c_int, cosine_mode: c_int, capacity: u64,
                                    d_out_a: *mut u64, d_out_b: *mut u64, d_out_keys: *mut u64, d_out_total: *mut u64, stream: *mut c_void) -> c_int;
        pub fn zh_cross_join_info(a: *const zh_index, out: *mut zh_cross_info) -> c_int;
        pub fn zh_knn_graph(idx: *mut zh_index, first_row: u64, n: u64, k: usize, metric: c_int, cosine_mode: c_int, out_ids: *mut u64,
                            out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_knn_graph_device(idx: *mut zh_index, first_row: u64, n: u64, k: usize, metric: c_int, cosine_mode: c_int, d_out_ids: *mut u64,
                                   d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_knn_graph_info(idx: *const zh_index, out: *mut zh_knn_info) -> c_int;
        pub fn zh_cross_knn(a: *mut zh_index, b: *mut zh_index, first_row: u64, n: u64, k: usize, metric: c_int, cosine_mode: c_int,
                            out_ids: *mut u64, out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_cross_knn_device(a: *mut zh_index, b: *mut zh_index, first_row: u64, n: u64, k: usize, metric: c_int, cosine_mode: c_int,
                                   d_out_ids: *mut u64, d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_cross_knn_info(a: *const zh_index, out: *mut zh_xknn_info) -> c_int;
        pub fn zh_knn_graph_forest(idx: *mut zh_index, first_row: u64, n: u64, k: usize, metric: c_int, cosine_mode: c_int, out_ids: *mut u64,
                                   out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_knn_graph_forest_device(idx: *mut zh_index, first_row: u64, n: u64, k: usize, metric: c_int, cosine_mode: c_int,
                                          d_out_ids: *mut u64, d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_knn_graph_forest_info(idx: *const zh_index, out: *mut zh_knn_forest_info) -> c_int;
        pub fn zh_knn_graph_refine(idx: *mut zh_index, in_ids: *const u64, in_counts: *const u32, in_k: usize, first_row: u64, n: u64, k: usize,
                                   metric: c_int, cosine_mode: c_int, out_ids: *mut u64, out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_knn_graph_refine_device(idx: *mut zh_index, d_in_ids: *const u64, d_in_counts: *const u32, in_k: usize, first_row: u64, n: u64,
                                          k: usize, metric: c_int, cosine_mode: c_int, d_out_ids: *mut u64, d_out_keys: *mut u64,
                                          d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_knn_graph_refine_info(idx: *const zh_index, out: *mut zh_knn_refine_info) -> c_int;
        pub fn zh_knn_graph_reverse(idx: *mut zh_index, in_ids: *const u64, in_counts: *const u32, in_k: usize, rev_k: usize, first_row: u64, n: u64,
                                    out_ids: *mut u64, out_counts: *mut u32, out_degree: *mut u32) -> c_int;
        pub fn zh_knn_graph_reverse_device(idx: *mut zh_index, d_in_ids: *const u64, d_in_counts: *const u32, in_k: usize, rev_k: usize, first_row: u64,
                                           n: u64, d_out_ids: *mut u64, d_out_counts: *mut u32, d_out_degree: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_knn_graph_reverse_info(idx: *const zh_index, out: *mut zh_knn_reverse_info) -> c_int;
        pub fn zh_knn_graph_refine_rev(idx: *mut zh_index, in_ids: *const u64, in_counts: *const u32, in_k: usize, rev_k: usize, first_row: u64, n: u64,
                                       k: usize, metric: c_int, cosine_mode: c_int, out_ids: *mut u64, out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_knn_graph_refine_rev_device(idx: *mut zh_index, d_in_ids: *const u64, d_in_counts: *const u32, in_k: usize, rev_k: usize,
                                              first_row: u64, n: u64, k: usize, metric: c_int, cosine_mode: c_int, d_out_ids: *mut u64,
                                              d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_knn_graph_refine_rev_info(idx: *const zh_index, out: *mut zh_knn_refine_rev_info) -> c_int;
        pub fn zh_knn_graph_prune(idx: *mut zh_index, in_ids: *const u64, in_counts: *const u32, in_k: usize, rev_k: usize, first_row: u64, n: u64,
                                  degree: usize, fill: c_int, metric: c_int, cosine_mode: c_int, out_ids: *mut u64, out_keys: *mut u64,
                                  out_counts: *mut u32) -> c_int;
        pub fn zh_knn_graph_prune_device(idx: *mut zh_index, d_in_ids: *const u64, d_in_counts: *const u32, in_k: usize, rev_k: usize,
                                         first_row: u64, n: u64, degree: usize, fill: c_int, metric: c_int, cosine_mode: c_int, d_out_ids: *mut u64,
                                         d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_knn_graph_prune_info(idx: *const zh_index, out: *mut zh_knn_prune_info) -> c_int;
        pub fn zh_knn_graph_descent(idx: *mut zh_index, in_ids: *const u64, in_counts: *const u32, in_k: usize, rev_k: usize, k: usize, rounds: usize,
                                    metric: c_int, cosine_mode: c_int, out_ids: *mut u64, out_keys: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_knn_graph_descent_device(idx: *mut zh_index, d_in_ids: *const u64, d_in_counts: *const u32, in_k: usize, rev_k: usize, k: usize,
                                           rounds: usize, metric: c_int, cosine_mode: c_int, d_out_ids: *mut u64, d_out_keys: *mut u64,
                                           d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_knn_graph_descent_info(idx: *const zh_index, out: *mut zh_knn_descent_info) -> c_int;
        pub fn zh_index_set_graph(idx: *mut zh_index, in_ids: *const u64, in_counts: *const u32, g_rows: u64, g_k: usize) -> c_int;
        pub fn zh_index_set_graph_device(idx: *mut zh_index, d_in_ids: *const u64, d_in_counts: *const u32, g_rows: u64, g_k: usize,
                                         stream: *mut c_void) -> c_int;
        pub fn zh_index_drop_graph(idx: *mut zh_index) -> c_int;
        pub fn zh_index_graph_info(idx: *const zh_index, out: *mut zh_graph_info) -> c_int;
        pub fn zh_search_graph_batch(idx: *mut zh_index, queries: *const f32, b: usize, seeds: *const u64, n_seed: usize, top_k: usize, beam: usize,
                                     width: usize, max_iters: usize, metric: c_int, cosine_mode: c_int, out_ids: *mut u64, out_keys: *mut u64,
                                     out_counts: *mut u32) -> c_int;
        pub fn zh_search_graph_batch_device(idx: *mut zh_index, d_queries: *const f32, b: usize, d_seeds: *const u64, n_seed: usize, top_k: usize,
                                            beam: usize, width: usize, max_iters: usize, metric: c_int, cosine_mode: c_int, d_out_ids: *mut u64,
                                            d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_search_graph_info(idx: *const zh_index, out: *mut zh_graph_search_info) -> c_int;
        pub fn zh_search_graph_filtered_batch(idx: *mut zh_index, queries: *const f32, b: usize, seeds: *const u64, n_seed: usize, top_k: usize,
                                              beam: usize, width: usize, max_iters: usize, metric: c_int, cosine_mode: c_int,
                                              filter_words: *const u32, n_bits: u64, out_ids: *mut u64, out_keys: *mut u64,
                                              out_counts: *mut u32) -> c_int;
        pub fn zh_search_graph_filtered_batch_device(idx: *mut zh_index, d_queries: *const f32, b: usize, d_seeds: *const u64, n_seed: usize,
                                                     top_k: usize, beam: usize, width: usize, max_iters: usize, metric: c_int, cosine_mode: c_int,
                                                     d_filter_words: *const u32, n_bits: u64, d_out_ids: *mut u64, d_out_keys: *mut u64,
                                                     d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_search_graph_filtered_info(idx: *const zh_index, out: *mut zh_graph_filtered_info) -> c_int;
        pub fn zh_search_graph_steered_batch(idx: *mut zh_index, queries: *const f32, b: usize, seeds: *const u64, n_seed: usize, top_k: usize,
                                             beam: usize, width: usize, max_iters: usize, metric: c_int, cosine_mode: c_int,
                                             filter_words: *const u32, n_bits: u64, hops: c_int, out_ids: *mut u64, out_keys: *mut u64,
                                             out_counts: *mut u32) -> c_int;
        pub fn zh_search_graph_steered_batch_device(idx: *mut zh_index, d_queries: *const f32, b: usize, d_seeds: *const u64, n_seed: usize,
                                                    top_k: usize, beam: usize, width: usize, max_iters: usize, metric: c_int, cosine_mode: c_int,
                                                    d_filter_words: *const u32, n_bits: u64, hops: c_int, d_out_ids: *mut u64,
                                                    d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_search_graph_steered_info(idx: *const zh_index, out: *mut zh_graph_steered_info) -> c_int;
        pub fn zh_index_extend_graph(idx: *mut zh_index, seeds: *const u64, n_new: u64, n_seed: usize, beam: usize, width: usize, max_iters: usize,
                                     batch: usize, metric: c_int, cosine_mode: c_int) -> c_int;
        pub fn zh_index_extend_graph_device(idx: *mut zh_index, d_seeds: *const u64, n_new: u64, n_seed: usize, beam: usize, width: usize,
                                            max_iters: usize, batch: usize, metric: c_int, cosine_mode: c_int, stream: *mut c_void) -> c_int;
        pub fn zh_index_extend_graph_info(idx: *const zh_index, out: *mut zh_graph_extend_info) -> c_int;
        pub fn zh_index_get_graph(idx: *mut zh_index, first_row: u64, n: u64, out_ids: *mut u64, out_counts: *mut u32) -> c_int;
        pub fn zh_index_get_graph_device(idx: *mut zh_index, first_row: u64, n: u64, d_out_ids: *mut u64, d_out_counts: *mut u32,
                                         stream: *mut c_void) -> c_int;
        pub fn zh_self_join_forest(idx: *mut zh_index, max_key: u64, metric: c_int, cosine_mode: c_int, capacity: u64, out_a: *mut u64,
                                   out_b: *mut u64, out_keys: *mut u64, out_total: *mut u64) -> c_int;
        pub fn zh_self_join_forest_device(idx: *mut zh_index, max_key: u64, metric: c_int, cosine_mode: c_int, capacity: u64, d_out_a: *mut u64,
                                          d_out_b: *mut u64, d_out_keys: *mut u64, d_out_total: *mut u64, stream: *mut c_void) -> c_int;
        pub fn zh_self_join_forest_info(idx: *const zh_index, out: *mut zh_join_forest_info) -> c_int;
        pub fn zh_search_range_forest_batch(idx: *mut zh_index, q: *const f32, b: usize, max_keys: *const u64, probe: u32, metric: c_int,
                                            cosine_mode: c_int, capacity: u64, out_offsets: *mut u64, out_ids: *mut u64, out_keys: *mut u64,
                                            out_total: *mut u64) -> c_int;
        pub fn zh_search_range_forest_batch_device(idx: *mut zh_index, d_q: *const f32, b: usize, d_max_keys: *const u64, probe: u32, metric: c_int,
                                                   cosine_mode: c_int, capacity: u64, d_out_offsets: *mut u64, d_out_ids: *mut u64,
                                                   d_out_keys: *mut u64, d_out_total: *mut u64, stream: *mut c_void) -> c_int;
        pub fn zh_search_range_forest_info(idx: *const zh_index, out: *mut zh_range_forest_info) -> c_int;
        pub fn zh_search_batch_device(idx: *mut zh_index, d_q: *const f32, b: usize, k: usize, metric: c_int, cosine_mode: c_int,
                                      d_out_ids: *mut u64, d_out_keys: *mut u64, d_out_counts: *mut u32, stream: *mut c_void) -> c_int;
        pub fn zh_distance_pair(metric: c_int, cosine_mode: c_int, a: *const f32, b: *const f32, dim: usize, out_key: *mut u64,
                                device: c_int) -> c_int;
        pub fn zh_merge_topk_device(device: c_int, n_shards: u32, b: usize, k: usize, d_ids: *const u64, d_keys: *const u64,
                                    d_counts: *const u32, d_out_ids: *mut u64, d_out_keys: *mut u64, d_out_counts: *mut u32,
                                    stream: *mut c_void) -> c_int;
        // the reference's on-disk tree values <-> flat forest; host code, no GPU
        pub fn zh_ref_forest_decode(dim: u32, n_trees: usize, values: *const *const u8, lens: *const usize, n_vectors: usize,
                                    uuids: *const u8, out: *mut *mut c_void, out_unknown_ids: *mut u64) -> c_int;
        pub fn zh_ref_forest_view(forest: *const c_void, out: *mut c_void /* zh_forest_view */) -> c_int;
        pub fn zh_ref_forest_free(forest: *mut c_void);
        pub fn zh_ref_tree_encode(forest: *const c_void /* zh_forest_view */, dim: u32, tree: u32, uuids: *const u8, n_rows: u64,
                                  out: *mut u8, cap: usize, out_len: *mut usize) -> c_int;
        pub fn zh_last_error() -> *const c_char;
        pub fn zh_trim_device_memory() -> c_int;
    }
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(ffi::zh_last_error()) }.to_string_lossy().into_owned()
}

fn check(rc: c_int) -> anyhow::Result<()> {
    if rc == 0 {
        return Ok(());
    }
    Err(anyhow::anyhow!("zebra_hip error {rc}: {}", last_error()))
}

/// Owns the device-side index.  `LSHIndex` is `Clone` in the reference (lsh.rs:144): clones share it.
struct HipIndex(*mut ffi::zh_index);
unsafe impl Send for HipIndex {}
unsafe impl Sync for HipIndex {} // search calls serialise inside the library
impl Drop for HipIndex {
    fn drop(&mut self) {
        unsafe { ffi::zh_index_destroy(self.0) }
    }
}

/// What a metric struct tells the index so that the batched search can run it on the device.  Every metric struct of
/// `src/distance.rs` implements it, so every call site of the reference compiles unchanged against
/// `search<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>` -- the reference's own bound
/// (lsh.rs:544-549) plus this one marker, which is the only addition to any public signature.
pub trait HipMetric {
    const METRIC: c_int;
    /// cosine mode for `CosineDistance`, `power` for Minkowski / p-norm, ignored otherwise
    fn param(&self) -> c_int {
        0
    }
}

macro_rules! simple_metric {
    ($name:ident, $code:expr, $doc:expr) => {
        #[doc = $doc]
        #[derive(Default, Debug, Clone)]
        pub struct $name<const N: usize>;
        impl<const N: usize> HipMetric for $name<N> {
            const METRIC: c_int = $code;
        }
        impl<const N: usize> Metric<Embedding<N>> for $name<N> {
            type Unit = DistanceUnit;
            fn distance(&self, a: &Embedding<N>, b: &Embedding<N>) -> DistanceUnit {
                // `Metric::distance` has no error channel (distance.rs:19-21): a failing device call must not read as key 0
                let mut key = 0u64;
                let rc = unsafe { ffi::zh_distance_pair($code, 0, a.as_ptr(), b.as_ptr(), N, &mut key, -1) };
                if rc != 0 {
                    panic!("zh_distance_pair({}): {}", stringify!($name), last_error());
                }
                key
            }
        }
    };
}
simple_metric!(CosineDistance, ffi::ZH_COSINE, "src/distance.rs:15-32 (key = bits of `1.0 - simsimd cosine`, literally)");
simple_metric!(L2SquaredDistance, ffi::ZH_L2SQ, "src/distance.rs:34-49");
simple_metric!(L2Distance, ffi::ZH_L2, "src/distance.rs:99-114");
simple_metric!(ChebyshevDistance, ffi::ZH_CHEBYSHEV, "src/distance.rs:51-61");
simple_metric!(CanberraDistance, ffi::ZH_CANBERRA, "src/distance.rs:63-73");
simple_metric!(BrayCurtisDistance, ffi::ZH_BRAY_CURTIS, "src/distance.rs:75-85");
simple_metric!(ManhattanDistance, ffi::ZH_MANHATTAN, "src/distance.rs:87-97");
simple_metric!(L3Distance, ffi::ZH_L3, "src/distance.rs:116-126");
simple_metric!(L4Distance, ffi::ZH_L4, "src/distance.rs:128-138");
simple_metric!(HammingDistance, ffi::ZH_HAMMING, "src/distance.rs:140-158");

/// src/distance.rs:160-174
#[derive(Default, Debug, Clone)]
pub struct MinkowskiDistance<const N: usize> {
    pub power: i32,
}
impl<const N: usize> HipMetric for MinkowskiDistance<N> {
    const METRIC: c_int = ffi::ZH_MINKOWSKI;
    fn param(&self) -> c_int {
        self.power
    }
}
/// src/distance.rs:176-190
#[derive(Default, Debug, Clone)]
pub struct PNormDistance<const N: usize> {
    pub power: i32,
}
impl<const N: usize> HipMetric for PNormDistance<N> {
    const METRIC: c_int = ffi::ZH_PNORM;
    fn param(&self) -> c_int {
        self.power
    }
}
macro_rules! power_metric {
    ($name:ident, $code:expr) => {
        impl<const N: usize> Metric<Embedding<N>> for $name<N> {
            type Unit = DistanceUnit;
            fn distance(&self, a: &Embedding<N>, b: &Embedding<N>) -> DistanceUnit {
                // every i32 power is served (the derived Default is 0); what can still fail is the device, and
                // `Metric::distance` has no error channel: fail loudly instead of returning key 0 for every pair
                let mut key = 0u64;
                let rc = unsafe { ffi::zh_distance_pair($code, self.power, a.as_ptr(), b.as_ptr(), N, &mut key, -1) };
                if rc != 0 {
                    panic!("zh_distance_pair({}, power {}): {}", stringify!($name), self.power, last_error());
                }
                key
            }
        }
    };
}
power_metric!(MinkowskiDistance, ffi::ZH_MINKOWSKI);
power_metric!(PNormDistance, ffi::ZH_PNORM);

/// lsh.rs:122-139
#[derive(Debug, Clone)]
pub struct LSHIndexOptions<const N: usize> {
    pub max_node_size: usize,
    pub num_trees: usize,
}
impl<const N: usize> Default for LSHIndexOptions<N> {
    fn default() -> Self {
        Self { max_node_size: 5, num_trees: 15 }
    }
}

/// `LSHIndex<N>` with the reference's public signatures (lsh.rs:144-565); ids are Uuids kept in a row table.
#[derive(Clone)]
pub struct LSHIndex<const N: usize> {
    hip: Arc<HipIndex>,
    ids: Arc<RwLock<IdTable>>,
}

/// row <-> Uuid (the library's ids are dense row numbers; Uuid::now_v7 at add time as in lsh.rs:415)
#[derive(Default)]
struct IdTable {
    of_row: Vec<Uuid>,
    row_of: HashMap<Uuid, u64>,
}

impl<const N: usize> LSHIndex<N> {
    pub fn new(_uuid: &Uuid, options: &LSHIndexOptions<N>) -> anyhow::Result<Self> {
        let mut o = unsafe { std::mem::zeroed::<ffi::zh_options>() };
        unsafe { ffi::zh_options_default(&mut o) };
        o.dim = N as u32;
        o.max_node_size = options.max_node_size as u32;
        o.num_trees = options.num_trees as u32;
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::zh_index_create(&o, &mut h) })?;
        Ok(Self { hip: Arc::new(HipIndex(h)), ids: Default::default() })
    }
    pub fn save(&self) -> anyhow::Result<()> {
        Ok(())
    }
    /// (new) zh_index_save: the index as ONE snapshot file (rows, removals, forest, the planes' sample rows), and the row -> Uuid table --
    /// which the library does not know -- beside it as `<path>.ids` (16 bytes per stored row, in row order; written to a temporary name and
    /// renamed, like the snapshot).  Holds the table across both, so the two files describe the same rows.  Needs the exclusion of `add`.
    pub fn save_snapshot(&self, path: &str) -> anyhow::Result<ffi::zh_snapshot_info> {
        let t = self.ids.write().unwrap();
        let c_path = std::ffi::CString::new(path)?;
        let mut info = ffi::zh_snapshot_info::default();
        check(unsafe { ffi::zh_index_save(self.hip.0, c_path.as_ptr(), &mut info) })?;
        anyhow::ensure!(info.stored_rows as usize == t.of_row.len(), "row table and snapshot disagree on the stored rows");
        let mut bytes = Vec::with_capacity(16 * t.of_row.len());
        for u in &t.of_row {
            bytes.extend_from_slice(u.as_bytes());
        }
        let tmp = format!("{path}.ids.tmp");
        std::fs::write(&tmp, &bytes)?;
        std::fs::File::open(&tmp)?.sync_all()?;
        std::fs::rename(&tmp, format!("{path}.ids"))?;
        Ok(info)
    }
    /// (new) zh_index_load + the row -> Uuid table written by `save_snapshot`: the saved index, for every later call.  Rows removed before the
    /// save keep their slot in the table (ids are row numbers) and stay unknown to `row_of`'s users exactly as before: the library refuses them.
    pub fn load(path: &str) -> anyhow::Result<Self> {
        let c_path = std::ffi::CString::new(path)?;
        let mut info = ffi::zh_snapshot_info::default();
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::zh_index_load(c_path.as_ptr(), -1, 0, &mut h, &mut info) })?;
        let hip = Arc::new(HipIndex(h)); // (dropped, and the index destroyed, on every early return below)
        anyhow::ensure!(info.dim as usize == N, "snapshot holds vectors of dimension {}, not {}", info.dim, N);
        let bytes = std::fs::read(format!("{path}.ids"))?;
        anyhow::ensure!(bytes.len() as u64 == 16 * info.stored_rows, "{path}.ids does not hold {} ids", info.stored_rows);
        let mut t = IdTable::default();
        for (row, b) in bytes.chunks_exact(16).enumerate() {
            let u = Uuid::from_slice(b)?;
            t.row_of.insert(u, row as u64);
            t.of_row.push(u);
        }
        Ok(Self { hip, ids: Arc::new(RwLock::new(t)) })
    }
    pub fn no_vectors(&self) -> bool {
        unsafe { ffi::zh_index_count(self.hip.0) == 0 }
    }
    pub fn no_trees(&self) -> bool {
        unsafe { ffi::zh_index_num_trees(self.hip.0) == 0 }
    }
    pub fn is_empty(&self) -> bool {
        self.no_vectors() || self.no_trees()
    }

    /// lsh.rs:440-466
    pub fn add(&self, embeddings: &Vec<Embedding<N>>) -> anyhow::Result<Vec<Uuid>> {
        let ids: Vec<Uuid> = embeddings.iter().map(|_| Uuid::now_v7()).collect();
        let mut t = self.ids.write().unwrap(); // rows are numbered in insertion order: hold the table across the call
        // The C layer stores the rows BEFORE it touches the trees and writes a row's id only once the row is stored; a failure
        // after that (a first build or an incremental insert that runs out of memory) keeps the rows -- their ids were handed
        // out.  So the row -> Uuid table follows what was STORED, not what succeeded: otherwise every later row would be
        // shifted against its Uuid (or `of_row[id]` would panic) once the index is rebuilt with zh_index_build.
        let mut rows = vec![u64::MAX; embeddings.len()];
        let rc = unsafe { ffi::zh_index_add(self.hip.0, embeddings.as_ptr() as *const f32, embeddings.len(), rows.as_mut_ptr()) };
        for (u, r) in ids.iter().zip(rows.iter()) {
            if *r != u64::MAX {
                t.row_of.insert(*u, t.of_row.len() as u64);
                t.of_row.push(*u);
            }
        }
        check(rc)?;
        Ok(ids)
    }

    /// lsh.rs:544-565
    pub fn search<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        query: &Embedding<N>,
        top_k: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, DistanceUnit)>> {
        Ok(self.search_batch(std::slice::from_ref(query), top_k, metric)?.pop().unwrap_or_default())
    }

    /// the rayon loop of core.rs:299-303 as one call
    pub fn search_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        top_k: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        let (mut ids, mut keys, mut counts) = (vec![0u64; b * top_k], vec![0u64; b * top_k], vec![0u32; b]);
        check(unsafe {
            ffi::zh_search_batch(self.hip.0, queries.as_ptr() as *const f32, b, top_k, Met::METRIC, metric.param(), ids.as_mut_ptr(),
                                 keys.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        let t = self.ids.read().unwrap();
        Ok((0..b).map(|i| (0..counts[i] as usize).map(|j| (t.of_row[ids[i * top_k + j] as usize], keys[i * top_k + j])).collect()).collect())
    }

    /// exact k nearest neighbours over every live stored row (zh_search_exact_batch): same keys and order as search_batch
    pub fn search_exact_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        top_k: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        let (mut ids, mut keys, mut counts) = (vec![0u64; b * top_k], vec![0u64; b * top_k], vec![0u32; b]);
        check(unsafe {
            ffi::zh_search_exact_batch(self.hip.0, queries.as_ptr() as *const f32, b, top_k, Met::METRIC, metric.param(), ids.as_mut_ptr(),
                                       keys.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        let t = self.ids.read().unwrap();
        Ok((0..b).map(|i| (0..counts[i] as usize).map(|j| (t.of_row[ids[i * top_k + j] as usize], keys[i * top_k + j])).collect()).collect())
    }

    /// (new) the exact k nearest neighbours among the vectors `allowed` names (zh_search_exact_filtered_batch): the answer of an index that
    /// held only those.  Unknown Uuids allow nothing; removed vectors are never returned.
    pub fn search_exact_filtered_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        top_k: usize,
        metric: &Met,
        allowed: &[Uuid],
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        let t = self.ids.read().unwrap();
        let n_bits = unsafe { ffi::zh_index_stored_rows(self.hip.0) };
        let mut words = vec![0u32; ((n_bits + 31) / 32) as usize];
        for row in allowed.iter().filter_map(|u| t.row_of.get(u).copied()).filter(|r| *r < n_bits) {
            words[(row >> 5) as usize] |= 1u32 << (row & 31);
        }
        let (mut ids, mut keys, mut counts) = (vec![0u64; b * top_k], vec![0u64; b * top_k], vec![0u32; b]);
        check(unsafe {
            ffi::zh_search_exact_filtered_batch(self.hip.0, queries.as_ptr() as *const f32, b, top_k, Met::METRIC, metric.param(),
                                                if n_bits > 0 { words.as_ptr() } else { std::ptr::null() }, n_bits, ids.as_mut_ptr(),
                                                keys.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        Ok((0..b).map(|i| (0..counts[i] as usize).map(|j| (t.of_row[ids[i * top_k + j] as usize], keys[i * top_k + j])).collect()).collect())
    }

    /// (new) every live vector whose key is <= the query's threshold key (zh_search_range_batch), ascending by (key, id): one call that
    /// counts (capacity 0), one that fetches.  `max_keys`: one DistanceUnit per query (u64::MAX = every live vector).
    pub fn search_range_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        max_keys: &[DistanceUnit],
        metric: &Met,
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        anyhow::ensure!(max_keys.len() == b, "search_range_batch: one threshold key per query");
        let t = self.ids.read().unwrap();
        let (mut offsets, mut total) = (vec![0u64; b + 1], 0u64);
        let rc = unsafe {
            ffi::zh_search_range_batch(self.hip.0, queries.as_ptr() as *const f32, b, max_keys.as_ptr(), Met::METRIC, metric.param(), 0,
                                       offsets.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), &mut total)
        };
        if rc != -5 {
            check(rc)?; // (-5 = ZH_ELIMIT: the hits exceed capacity 0; offsets and total are exact)
        }
        let (mut ids, mut keys) = (vec![0u64; total as usize + 1], vec![0u64; total as usize + 1]);
        if total > 0 {
            check(unsafe {
                ffi::zh_search_range_batch(self.hip.0, queries.as_ptr() as *const f32, b, max_keys.as_ptr(), Met::METRIC, metric.param(), total,
                                           offsets.as_mut_ptr(), ids.as_mut_ptr(), keys.as_mut_ptr(), &mut total)
            })?;
        }
        Ok((0..b).map(|i| (offsets[i] as usize..offsets[i + 1] as usize).map(|j| (t.of_row[ids[j] as usize], keys[j])).collect()).collect())
    }

    /// (new) the forest range search (zh_search_range_forest_batch): search_range_batch's hits among the members of the leaves the walk visits for
    /// each query with n = `probe` (1: the leaf the query hashes to in each tree); exact keys on an approximate candidate set, each hit once.
    /// One call that counts (capacity 0), one that fetches.  Needs a built forest.
    pub fn search_range_forest_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        max_keys: &[DistanceUnit],
        probe: u32,
        metric: &Met,
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        anyhow::ensure!(max_keys.len() == b, "search_range_forest_batch: one threshold key per query");
        let t = self.ids.read().unwrap();
        let (mut offsets, mut total) = (vec![0u64; b + 1], 0u64);
        let rc = unsafe {
            ffi::zh_search_range_forest_batch(self.hip.0, queries.as_ptr() as *const f32, b, max_keys.as_ptr(), probe, Met::METRIC, metric.param(), 0,
                                              offsets.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), &mut total)
        };
        if rc != -5 {
            check(rc)?; // (-5 = ZH_ELIMIT: the hits exceed capacity 0; offsets and total are exact)
        }
        let (mut ids, mut keys) = (vec![0u64; total as usize + 1], vec![0u64; total as usize + 1]);
        if total > 0 {
            check(unsafe {
                ffi::zh_search_range_forest_batch(self.hip.0, queries.as_ptr() as *const f32, b, max_keys.as_ptr(), probe, Met::METRIC, metric.param(),
                                                  total, offsets.as_mut_ptr(), ids.as_mut_ptr(), keys.as_mut_ptr(), &mut total)
            })?;
        }
        Ok((0..b).map(|i| (offsets[i] as usize..offsets[i + 1] as usize).map(|j| (t.of_row[ids[j] as usize], keys[j])).collect()).collect())
    }

    /// what the most recent forest range search did (zh_search_range_forest_info)
    pub fn range_forest_info(&self) -> anyhow::Result<ffi::zh_range_forest_info> {
        let mut info = ffi::zh_range_forest_info::default();
        check(unsafe { ffi::zh_search_range_forest_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) every pair of distinct live vectors (a, b), a before b by row, whose key (stored b against a query equal to a) is <= `max_key`
    /// (zh_self_join), ascending by (a, key, b): one call that counts (capacity 0), one that fetches.  u64::MAX = every pair.
    pub fn self_join<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        max_key: DistanceUnit,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Uuid, DistanceUnit)>> {
        let t = self.ids.read().unwrap();
        let mut total = 0u64;
        let rc = unsafe {
            ffi::zh_self_join(self.hip.0, max_key, Met::METRIC, metric.param(), 0, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(),
                              &mut total)
        };
        if rc != -5 {
            check(rc)?;
        }
        let n = total as usize + 1;
        let (mut a, mut b, mut keys) = (vec![0u64; n], vec![0u64; n], vec![0u64; n]);
        if total > 0 {
            check(unsafe {
                ffi::zh_self_join(self.hip.0, max_key, Met::METRIC, metric.param(), total, a.as_mut_ptr(), b.as_mut_ptr(), keys.as_mut_ptr(), &mut total)
            })?;
        }
        Ok((0..total as usize).map(|i| (t.of_row[a[i] as usize], t.of_row[b[i] as usize], keys[i])).collect())
    }

    /// (new) the join between two indexes (zh_cross_join): every pair (live vector a of self, live vector b of `other`) whose key -- that of
    /// stored b against a query equal to a -- is <= `max_key`, ascending by (a, key, b): one call that counts (capacity 0), one that fetches.
    /// u64::MAX = every pair of the rectangle.  The library takes both indexes' locks together; `self` and `other` must be different indexes.
    pub fn cross_join<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        other: &Self,
        max_key: DistanceUnit,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Uuid, DistanceUnit)>> {
        let ta = self.ids.read().unwrap();
        let tb = other.ids.read().unwrap();
        let mut total = 0u64;
        let rc = unsafe {
            ffi::zh_cross_join(self.hip.0, other.hip.0, max_key, Met::METRIC, metric.param(), 0, std::ptr::null_mut(), std::ptr::null_mut(),
                               std::ptr::null_mut(), &mut total)
        };
        if rc != -5 {
            check(rc)?;
        }
        let n = total as usize + 1;
        let (mut a, mut b, mut keys) = (vec![0u64; n], vec![0u64; n], vec![0u64; n]);
        if total > 0 {
            check(unsafe {
                ffi::zh_cross_join(self.hip.0, other.hip.0, max_key, Met::METRIC, metric.param(), total, a.as_mut_ptr(), b.as_mut_ptr(),
                                   keys.as_mut_ptr(), &mut total)
            })?;
        }
        Ok((0..total as usize).map(|i| (ta.of_row[a[i] as usize], tb.of_row[b[i] as usize], keys[i])).collect())
    }

    /// what the most recent cross_join with this index on the left did (zh_cross_join_info)
    pub fn cross_info(&self) -> anyhow::Result<ffi::zh_cross_info> {
        let mut info = ffi::zh_cross_info::default();
        check(unsafe { ffi::zh_cross_join_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) the exact k-NN graph (zh_knn_graph): per stored vector, in row order, its `k` nearest OTHER live vectors by (key, row), the key that
    /// of the neighbour against a query equal to the vector; a removed vector's list is empty.  Fetched in slabs of 65536 rows.
    pub fn knn_graph<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Vec<(Uuid, DistanceUnit)>)>> {
        const SLAB: u64 = 65536;
        let t = self.ids.read().unwrap();
        let stored = t.of_row.len() as u64;
        let mut out = Vec::with_capacity(stored as usize);
        let (mut ids, mut keys, mut counts) = (vec![0u64; SLAB as usize * k + 1], vec![0u64; SLAB as usize * k + 1], vec![0u32; SLAB as usize]);
        let mut first = 0u64;
        while first < stored {
            let n = SLAB.min(stored - first);
            check(unsafe {
                ffi::zh_knn_graph(self.hip.0, first, n, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(), counts.as_mut_ptr())
            })?;
            for i in 0..n as usize {
                let line = (0..counts[i] as usize).map(|j| (t.of_row[ids[i * k + j] as usize], keys[i * k + j])).collect();
                out.push((t.of_row[first as usize + i], line));
            }
            first += n;
        }
        Ok(out)
    }

    /// (new) the k-NN join between two indexes (zh_cross_knn): per stored vector of self, in row order, its `k` nearest live vectors of `other`
    /// by (key, row) -- the key that of other's stored vector against a query equal to the vector, other's exact search bit for bit; nothing is
    /// excluded; a removed vector's list is empty.  Fetched in slabs of 65536 rows.  `self` and `other` must be different indexes.
    pub fn cross_knn<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        other: &Self,
        k: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Vec<(Uuid, DistanceUnit)>)>> {
        const SLAB: u64 = 65536;
        let ta = self.ids.read().unwrap();
        let tb = other.ids.read().unwrap();
        let stored = ta.of_row.len() as u64;
        let mut out = Vec::with_capacity(stored as usize);
        let (mut ids, mut keys, mut counts) = (vec![0u64; SLAB as usize * k + 1], vec![0u64; SLAB as usize * k + 1], vec![0u32; SLAB as usize]);
        let mut first = 0u64;
        while first < stored {
            let n = SLAB.min(stored - first);
            check(unsafe {
                ffi::zh_cross_knn(self.hip.0, other.hip.0, first, n, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(),
                                  counts.as_mut_ptr())
            })?;
            for i in 0..n as usize {
                let line = (0..counts[i] as usize).map(|j| (tb.of_row[ids[i * k + j] as usize], keys[i * k + j])).collect();
                out.push((ta.of_row[first as usize + i], line));
            }
            first += n;
        }
        Ok(out)
    }

    /// what the most recent cross_knn with this index on the left did (zh_cross_knn_info)
    pub fn cross_knn_info(&self) -> anyhow::Result<ffi::zh_xknn_info> {
        let mut info = ffi::zh_xknn_info::default();
        check(unsafe { ffi::zh_cross_knn_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) the forest k-NN graph (zh_knn_graph_forest): knn_graph's shape, a vector's candidates being the vectors that share a leaf with it in
    /// some tree; a removed vector's list and that of a vector no tree holds are empty.  Fetched in slabs of 1 048 576 rows.
    pub fn knn_graph_forest<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Vec<(Uuid, DistanceUnit)>)>> {
        const SLAB: u64 = 1 << 20;
        let t = self.ids.read().unwrap();
        let stored = t.of_row.len() as u64;
        let mut out = Vec::with_capacity(stored as usize);
        let cap = SLAB.min(stored) as usize;
        let (mut ids, mut keys, mut counts) = (vec![0u64; cap * k + 1], vec![0u64; cap * k + 1], vec![0u32; cap + 1]);
        let mut first = 0u64;
        while first < stored {
            let n = SLAB.min(stored - first);
            check(unsafe {
                ffi::zh_knn_graph_forest(self.hip.0, first, n, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(), counts.as_mut_ptr())
            })?;
            for i in 0..n as usize {
                let line = (0..counts[i] as usize).map(|j| (t.of_row[ids[i * k + j] as usize], keys[i * k + j])).collect();
                out.push((t.of_row[first as usize + i], line));
            }
            first += n;
        }
        Ok(out)
    }

    /// (new) the refined forest k-NN graph (zh_knn_graph_forest, then zh_knn_graph_refine): the forest graph of the whole table in row numbers,
    /// then up to `rounds` join rounds -- each vector's neighbours and their neighbours, ranked by the exact key -- each round's output the next
    /// round's input, stopping early once a round changes nothing (`updates` == 0).  knn_graph's shape.
    pub fn knn_graph_refined<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        rounds: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Vec<(Uuid, DistanceUnit)>)>> {
        self.knn_graph_refined_rev(k, rounds, 0, metric)
    }

    /// (new) knn_graph_refined with up to `reverse` sampled reverse neighbours of every vector -- the vectors that name it, picked by a hash of
    /// the pair -- and THEIR lists among each round's candidates (zh_knn_graph_refine_rev; k + reverse <= 64).  reverse == 0 is
    /// knn_graph_refined's call and path exactly.
    pub fn knn_graph_refined_rev<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        rounds: usize,
        reverse: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Vec<(Uuid, DistanceUnit)>)>> {
        let t = self.ids.read().unwrap();
        let stored = t.of_row.len();
        let (mut ids, mut keys, mut counts) = (vec![0u64; stored * k + 1], vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        if stored > 0 {
            check(unsafe {
                ffi::zh_knn_graph_forest(self.hip.0, 0, stored as u64, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(),
                                         counts.as_mut_ptr())
            })?;
        }
        let (mut rids, mut rcounts) = (vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        for _ in 0..rounds {
            if stored == 0 || k == 0 {
                break;
            }
            let updates = if reverse == 0 {
                check(unsafe {
                    ffi::zh_knn_graph_refine(self.hip.0, ids.as_ptr(), counts.as_ptr(), k, 0, stored as u64, k, Met::METRIC, metric.param(),
                                             rids.as_mut_ptr(), keys.as_mut_ptr(), rcounts.as_mut_ptr())
                })?;
                self.knn_refine_info()?.updates
            } else {
                check(unsafe {
                    ffi::zh_knn_graph_refine_rev(self.hip.0, ids.as_ptr(), counts.as_ptr(), k, reverse, 0, stored as u64, k, Met::METRIC,
                                                 metric.param(), rids.as_mut_ptr(), keys.as_mut_ptr(), rcounts.as_mut_ptr())
                })?;
                self.knn_refine_rev_info()?.updates
            };
            std::mem::swap(&mut ids, &mut rids);
            std::mem::swap(&mut counts, &mut rcounts);
            if updates == 0 {
                break;
            }
        }
        Ok((0..stored)
            .map(|i| (t.of_row[i], (0..counts[i] as usize).map(|j| (t.of_row[ids[i * k + j] as usize], keys[i * k + j])).collect()))
            .collect())
    }

    /// (new) knn_graph_refined_rev's answer from ONE call that runs the rounds on the device and, from the second round on, keys only what a new
    /// entry of a line brings up (zh_knn_graph_descent; 1 <= rounds <= 32, 1 <= k, k + reverse <= 64)
    pub fn knn_graph_descent<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        rounds: usize,
        reverse: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Vec<(Uuid, DistanceUnit)>)>> {
        let t = self.ids.read().unwrap();
        let stored = t.of_row.len();
        let (mut ids, mut keys, mut counts) = (vec![0u64; stored * k + 1], vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        let (mut rids, mut rcounts) = (vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        if stored > 0 {
            check(unsafe {
                ffi::zh_knn_graph_forest(self.hip.0, 0, stored as u64, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(),
                                         counts.as_mut_ptr())
            })?;
            check(unsafe {
                ffi::zh_knn_graph_descent(self.hip.0, ids.as_ptr(), counts.as_ptr(), k, reverse, k, rounds, Met::METRIC, metric.param(),
                                          rids.as_mut_ptr(), keys.as_mut_ptr(), rcounts.as_mut_ptr())
            })?;
        }
        Ok((0..stored)
            .map(|i| (t.of_row[i], (0..rcounts[i] as usize).map(|j| (t.of_row[rids[i * k + j] as usize], keys[i * k + j])).collect()))
            .collect())
    }

    /// (new) knn_graph_descent's graph pruned by the occlusion rule of the graph indexes (zh_knn_graph_prune): of each vector's k neighbours and
    /// up to `reverse` sampled reverse neighbours, in (key, id) order, one is kept unless a neighbour kept before it is closer to it than the
    /// vector itself; at most `degree` are kept, and with `fill` a line that came short takes the first dropped ones.  degree, k + reverse <= 64
    pub fn knn_graph_pruned<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        rounds: usize,
        reverse: usize,
        degree: usize,
        fill: bool,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Vec<(Uuid, DistanceUnit)>)>> {
        let t = self.ids.read().unwrap();
        let stored = t.of_row.len();
        let (mut ids, mut keys, mut counts) = (vec![0u64; stored * k + 1], vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        let (mut rids, mut rcounts) = (vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        let (mut pids, mut pkeys, mut pcounts) = (vec![0u64; stored * degree + 1], vec![0u64; stored * degree + 1], vec![0u32; stored + 1]);
        if stored > 0 {
            check(unsafe {
                ffi::zh_knn_graph_forest(self.hip.0, 0, stored as u64, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(),
                                         counts.as_mut_ptr())
            })?;
            check(unsafe {
                ffi::zh_knn_graph_descent(self.hip.0, ids.as_ptr(), counts.as_ptr(), k, reverse, k, rounds, Met::METRIC, metric.param(),
                                          rids.as_mut_ptr(), keys.as_mut_ptr(), rcounts.as_mut_ptr())
            })?;
            check(unsafe {
                ffi::zh_knn_graph_prune(self.hip.0, rids.as_ptr(), rcounts.as_ptr(), k, reverse, 0, stored as u64, degree, fill as c_int, Met::METRIC,
                                        metric.param(), pids.as_mut_ptr(), pkeys.as_mut_ptr(), pcounts.as_mut_ptr())
            })?;
        }
        Ok((0..stored)
            .map(|i| (t.of_row[i], (0..pcounts[i] as usize).map(|j| (t.of_row[pids[i * degree + j] as usize], pkeys[i * degree + j])).collect()))
            .collect())
    }

    /// what the most recent pruning call did (zh_knn_graph_prune_info)
    pub fn knn_prune_info(&self) -> anyhow::Result<ffi::zh_knn_prune_info> {
        let mut info = ffi::zh_knn_prune_info::default();
        check(unsafe { ffi::zh_knn_graph_prune_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) make the graph `search_graph_batch` walks and keep it on the device: the forest graph, NN-descent (knn_graph_descent's calls), then
    /// zh_index_set_graph over every stored row.  Vectors added later are found only as seeds until extend_graph (or the next build_graph); removed ones are
    /// skipped at once; compact() and clear() drop the graph
    pub fn build_graph<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        rounds: usize,
        reverse: usize,
        metric: &Met,
    ) -> anyhow::Result<ffi::zh_graph_info> {
        let t = self.ids.read().unwrap();
        let stored = t.of_row.len();
        let (mut ids, mut keys, mut counts) = (vec![0u64; stored * k + 1], vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        let (mut rids, mut rcounts) = (vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        if stored > 0 {
            check(unsafe {
                ffi::zh_knn_graph_forest(self.hip.0, 0, stored as u64, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(),
                                         counts.as_mut_ptr())
            })?;
            check(unsafe {
                ffi::zh_knn_graph_descent(self.hip.0, ids.as_ptr(), counts.as_ptr(), k, reverse, k, rounds, Met::METRIC, metric.param(),
                                          rids.as_mut_ptr(), keys.as_mut_ptr(), rcounts.as_mut_ptr())
            })?;
        }
        check(unsafe { ffi::zh_index_set_graph(self.hip.0, rids.as_ptr(), rcounts.as_ptr(), stored as u64, k) })?;
        self.graph_info()
    }

    /// (new) lines for the vectors added since build_graph (or the last extend_graph), and the old lines re-ranked to name them
    /// (zh_index_extend_graph): every new vector starts its walk from the same n_seed strided rows of the graph before the call; the new rows go in
    /// chunks of `batch` (<= 1024), and the rows of one chunk never name each other.  k <= beam
    #[allow(clippy::too_many_arguments)]
    pub fn extend_graph<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        beam: usize,
        width: usize,
        max_iters: usize,
        n_seed: usize,
        batch: usize,
        metric: &Met,
    ) -> anyhow::Result<ffi::zh_graph_extend_info> {
        let _t = self.ids.read().unwrap();
        let g_rows = self.graph_info()?.g_rows;
        let n_new = unsafe { ffi::zh_index_stored_rows(self.hip.0) }.saturating_sub(g_rows);
        let seeds: Vec<u64> = (0..n_new as usize * n_seed).map(|i| ((i % n_seed) as u64) * g_rows / n_seed.max(1) as u64).collect();
        check(unsafe {
            ffi::zh_index_extend_graph(self.hip.0, if n_new > 0 { seeds.as_ptr() } else { std::ptr::null() }, n_new, n_seed, beam, width, max_iters, batch,
                                       Met::METRIC, metric.param())
        })?;
        let mut info = ffi::zh_graph_extend_info::default();
        check(unsafe { ffi::zh_index_extend_graph_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) the attached table read back as rows (zh_index_get_graph): per stored row of the graph the rows its line names, in table order
    pub fn get_graph(&self) -> anyhow::Result<Vec<Vec<u64>>> {
        let g = self.graph_info()?;
        let (n, k) = (g.g_rows as usize, g.g_k as usize);
        let (mut ids, mut counts) = (vec![0u64; n * k + 1], vec![0u32; n + 1]);
        check(unsafe { ffi::zh_index_get_graph(self.hip.0, 0, n as u64, ids.as_mut_ptr(), counts.as_mut_ptr()) })?;
        Ok((0..n).map(|i| ids[i * k..i * k + counts[i] as usize].to_vec()).collect())
    }

    /// (new) release the attached graph (zh_index_drop_graph)
    pub fn drop_graph(&self) -> anyhow::Result<()> {
        check(unsafe { ffi::zh_index_drop_graph(self.hip.0) })
    }

    /// (new) the attached graph (zh_index_graph_info)
    pub fn graph_info(&self) -> anyhow::Result<ffi::zh_graph_info> {
        let mut info = ffi::zh_graph_info::default();
        check(unsafe { ffi::zh_index_graph_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) beam search over the attached graph under search_exact_batch's keys (zh_search_graph_batch): every query starts from the same n_seed
    /// strided rows of the graph; the beam keeps the `beam` best vectors met, an iteration expands its first `width` unexpanded ones, until none
    /// is left or max_iters (0: no cap) iterations ran.  1 <= top_k <= beam <= 256, width * k <= 256, n_seed <= 64
    #[allow(clippy::too_many_arguments)]
    pub fn search_graph_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        top_k: usize,
        beam: usize,
        width: usize,
        max_iters: usize,
        n_seed: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        let g_rows = self.graph_info()?.g_rows;
        let seeds: Vec<u64> = (0..b * n_seed).map(|i| ((i % n_seed) as u64) * g_rows / n_seed.max(1) as u64).collect();
        let (mut ids, mut keys, mut counts) = (vec![0u64; b * top_k + 1], vec![0u64; b * top_k + 1], vec![0u32; b + 1]);
        check(unsafe {
            ffi::zh_search_graph_batch(self.hip.0, queries.as_ptr() as *const f32, b, seeds.as_ptr(), n_seed, top_k, beam, width, max_iters,
                                       Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        let t = self.ids.read().unwrap();
        Ok((0..b).map(|i| (0..counts[i] as usize).map(|j| (t.of_row[ids[i * top_k + j] as usize], keys[i * top_k + j])).collect()).collect())
    }

    /// (new) search_graph_batch's walk -- through every live vector -- answered with the nearest of the vectors it keyed that `allowed` names
    /// (zh_search_graph_filtered_batch).  Unknown Uuids allow nothing; removed vectors are neither walked nor returned.  With every vector
    /// allowed it is search_graph_batch's answer
    #[allow(clippy::too_many_arguments)]
    pub fn search_graph_filtered_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        top_k: usize,
        beam: usize,
        width: usize,
        max_iters: usize,
        n_seed: usize,
        metric: &Met,
        allowed: &[Uuid],
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        let g_rows = self.graph_info()?.g_rows;
        let seeds: Vec<u64> = (0..b * n_seed).map(|i| ((i % n_seed) as u64) * g_rows / n_seed.max(1) as u64).collect();
        let t = self.ids.read().unwrap();
        let n_bits = unsafe { ffi::zh_index_stored_rows(self.hip.0) };
        let mut words = vec![0u32; ((n_bits + 31) / 32) as usize];
        for row in allowed.iter().filter_map(|u| t.row_of.get(u).copied()).filter(|r| *r < n_bits) {
            words[(row >> 5) as usize] |= 1u32 << (row & 31);
        }
        let (mut ids, mut keys, mut counts) = (vec![0u64; b * top_k + 1], vec![0u64; b * top_k + 1], vec![0u32; b + 1]);
        check(unsafe {
            ffi::zh_search_graph_filtered_batch(self.hip.0, queries.as_ptr() as *const f32, b, seeds.as_ptr(), n_seed, top_k, beam, width, max_iters,
                                                Met::METRIC, metric.param(), if n_bits > 0 { words.as_ptr() } else { std::ptr::null() }, n_bits,
                                                ids.as_mut_ptr(), keys.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        Ok((0..b).map(|i| (0..counts[i] as usize).map(|j| (t.of_row[ids[i * top_k + j] as usize], keys[i * top_k + j])).collect()).collect())
    }

    /// (new) a walk that sees the filter (zh_search_graph_steered_batch): the beam holds only vectors `allowed` names; with hops = 2 a vector
    /// that is not allowed is hopped over -- the allowed entries of its line are candidates, at most 256 an iteration.  The seeds are n_seed
    /// rows strided over the allowed ones (a seed that is not allowed would be ignored).  hops is 1 or 2.  With every vector allowed it is
    /// search_graph_batch's answer
    #[allow(clippy::too_many_arguments)]
    pub fn search_graph_steered_batch<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        queries: &[Embedding<N>],
        top_k: usize,
        beam: usize,
        width: usize,
        max_iters: usize,
        n_seed: usize,
        metric: &Met,
        allowed: &[Uuid],
        hops: i32,
    ) -> anyhow::Result<Vec<Vec<(Uuid, DistanceUnit)>>> {
        let b = queries.len();
        let t = self.ids.read().unwrap();
        let n_bits = unsafe { ffi::zh_index_stored_rows(self.hip.0) };
        let mut words = vec![0u32; ((n_bits + 31) / 32) as usize];
        let mut rows: Vec<u64> = allowed.iter().filter_map(|u| t.row_of.get(u).copied()).filter(|r| *r < n_bits).collect();
        rows.sort_unstable();
        rows.dedup();
        for row in rows.iter() {
            words[(row >> 5) as usize] |= 1u32 << (row & 31);
        }
        let line: Vec<u64> = (0..n_seed).map(|j| if rows.is_empty() { u64::MAX } else { rows[(j * rows.len() / n_seed.max(1)) % rows.len()] }).collect();
        let seeds: Vec<u64> = (0..b * n_seed).map(|i| line[i % n_seed]).collect();
        let (mut ids, mut keys, mut counts) = (vec![0u64; b * top_k + 1], vec![0u64; b * top_k + 1], vec![0u32; b + 1]);
        check(unsafe {
            ffi::zh_search_graph_steered_batch(self.hip.0, queries.as_ptr() as *const f32, b, seeds.as_ptr(), n_seed, top_k, beam, width, max_iters,
                                               Met::METRIC, metric.param(), if n_bits > 0 { words.as_ptr() } else { std::ptr::null() }, n_bits,
                                               hops, ids.as_mut_ptr(), keys.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        Ok((0..b).map(|i| (0..counts[i] as usize).map(|j| (t.of_row[ids[i * top_k + j] as usize], keys[i * top_k + j])).collect()).collect())
    }

    /// what the most recent zh_search_graph_steered_batch call did (zh_search_graph_steered_info)
    pub fn search_graph_steered_info(&self) -> anyhow::Result<ffi::zh_graph_steered_info> {
        let mut info = ffi::zh_graph_steered_info::default();
        check(unsafe { ffi::zh_search_graph_steered_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent zh_search_graph_filtered_batch call did (zh_search_graph_filtered_info)
    pub fn search_graph_filtered_info(&self) -> anyhow::Result<ffi::zh_graph_filtered_info> {
        let mut info = ffi::zh_graph_filtered_info::default();
        check(unsafe { ffi::zh_search_graph_filtered_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent zh_search_graph_batch call did, summed over its queries (zh_search_graph_info)
    pub fn search_graph_info(&self) -> anyhow::Result<ffi::zh_graph_search_info> {
        let mut info = ffi::zh_graph_search_info::default();
        check(unsafe { ffi::zh_search_graph_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent zh_knn_graph_descent call did, round by round (zh_knn_graph_descent_info)
    pub fn knn_descent_info(&self) -> anyhow::Result<ffi::zh_knn_descent_info> {
        let mut info = ffi::zh_knn_descent_info::default();
        check(unsafe { ffi::zh_knn_graph_descent_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent graph refinement call did (zh_knn_graph_refine_info)
    pub fn knn_refine_info(&self) -> anyhow::Result<ffi::zh_knn_refine_info> {
        let mut info = ffi::zh_knn_refine_info::default();
        check(unsafe { ffi::zh_knn_graph_refine_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent refinement with reverse neighbours did (zh_knn_graph_refine_rev_info)
    pub fn knn_refine_rev_info(&self) -> anyhow::Result<ffi::zh_knn_refine_rev_info> {
        let mut info = ffi::zh_knn_refine_rev_info::default();
        check(unsafe { ffi::zh_knn_graph_refine_rev_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) every vector's in-degree in the forest k-NN graph (zh_knn_graph_forest, then zh_knn_graph_reverse): how many other vectors name it
    /// among their k leaf-mate neighbours -- the hubness score
    pub fn knn_in_degrees<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        k: usize,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, u32)>> {
        let t = self.ids.read().unwrap();
        let stored = t.of_row.len();
        if stored == 0 || k == 0 {
            return Ok(Vec::new());
        }
        let (mut ids, mut keys, mut counts) = (vec![0u64; stored * k + 1], vec![0u64; stored * k + 1], vec![0u32; stored + 1]);
        check(unsafe {
            ffi::zh_knn_graph_forest(self.hip.0, 0, stored as u64, k, Met::METRIC, metric.param(), ids.as_mut_ptr(), keys.as_mut_ptr(),
                                     counts.as_mut_ptr())
        })?;
        let (mut rids, mut rcounts, mut degree) = (vec![0u64; stored + 1], vec![0u32; stored + 1], vec![0u32; stored + 1]);
        check(unsafe {
            ffi::zh_knn_graph_reverse(self.hip.0, ids.as_ptr(), counts.as_ptr(), k, 1, 0, stored as u64, rids.as_mut_ptr(), rcounts.as_mut_ptr(),
                                      degree.as_mut_ptr())
        })?;
        Ok((0..stored).map(|i| (t.of_row[i], degree[i])).collect())
    }

    /// what the most recent zh_knn_graph_reverse call did (zh_knn_graph_reverse_info)
    pub fn knn_reverse_info(&self) -> anyhow::Result<ffi::zh_knn_reverse_info> {
        let mut info = ffi::zh_knn_reverse_info::default();
        check(unsafe { ffi::zh_knn_graph_reverse_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// (new) the forest self-join (zh_self_join_forest): self_join's pairs among the vectors that share a leaf in at least one tree, each pair
    /// once, ascending by (a, key, b); exact keys on an approximate candidate set.  One call that counts (capacity 0), one that fetches.
    pub fn self_join_forest<Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Send + Sync>(
        &self,
        max_key: DistanceUnit,
        metric: &Met,
    ) -> anyhow::Result<Vec<(Uuid, Uuid, DistanceUnit)>> {
        let t = self.ids.read().unwrap();
        let mut total = 0u64;
        let rc = unsafe {
            ffi::zh_self_join_forest(self.hip.0, max_key, Met::METRIC, metric.param(), 0, std::ptr::null_mut(), std::ptr::null_mut(),
                                     std::ptr::null_mut(), &mut total)
        };
        if rc != -5 {
            check(rc)?;
        }
        let n = total as usize + 1;
        let (mut a, mut b, mut keys) = (vec![0u64; n], vec![0u64; n], vec![0u64; n]);
        if total > 0 {
            check(unsafe {
                ffi::zh_self_join_forest(self.hip.0, max_key, Met::METRIC, metric.param(), total, a.as_mut_ptr(), b.as_mut_ptr(), keys.as_mut_ptr(),
                                         &mut total)
            })?;
        }
        Ok((0..total as usize).map(|i| (t.of_row[a[i] as usize], t.of_row[b[i] as usize], keys[i])).collect())
    }

    /// what the most recent forest self-join did (zh_self_join_forest_info)
    pub fn join_forest_info(&self) -> anyhow::Result<ffi::zh_join_forest_info> {
        let mut info = ffi::zh_join_forest_info::default();
        check(unsafe { ffi::zh_self_join_forest_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent forest k-NN graph call did (zh_knn_graph_forest_info)
    pub fn knn_forest_info(&self) -> anyhow::Result<ffi::zh_knn_forest_info> {
        let mut info = ffi::zh_knn_forest_info::default();
        check(unsafe { ffi::zh_knn_graph_forest_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent k-NN graph call did (zh_knn_graph_info)
    pub fn knn_info(&self) -> anyhow::Result<ffi::zh_knn_info> {
        let mut info = ffi::zh_knn_info::default();
        check(unsafe { ffi::zh_knn_graph_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent self-join did (zh_self_join_info)
    pub fn join_info(&self) -> anyhow::Result<ffi::zh_join_info> {
        let mut info = ffi::zh_join_info::default();
        check(unsafe { ffi::zh_self_join_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent range search did (zh_search_range_info)
    pub fn range_info(&self) -> anyhow::Result<ffi::zh_range_info> {
        let mut info = ffi::zh_range_info::default();
        check(unsafe { ffi::zh_search_range_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// what the most recent filtered search did (zh_search_filtered_info)
    pub fn filtered_info(&self) -> anyhow::Result<ffi::zh_filtered_info> {
        let mut info = ffi::zh_filtered_info::default();
        check(unsafe { ffi::zh_search_filtered_info(self.hip.0, &mut info) })?;
        Ok(info)
    }

    /// lsh.rs:473-503 (as intended: the ids leave every tree)
    pub fn remove(&self, embedding_ids: &Vec<Uuid>) -> anyhow::Result<DashSet<Uuid>> {
        let t = self.ids.read().unwrap();
        let rows: Vec<u64> = embedding_ids.iter().filter_map(|u| t.row_of.get(u).copied()).collect(); // O(1) per id
        let mut found = vec![0u8; rows.len()];
        check(unsafe { ffi::zh_index_remove(self.hip.0, rows.as_ptr(), rows.len(), found.as_mut_ptr(), std::ptr::null_mut()) })?;
        let removed = DashSet::new();
        for (r, f) in rows.iter().zip(found) {
            if f != 0 {
                removed.insert(t.of_row[*r as usize]);
            }
        }
        Ok(removed)
    }

    /// lsh.rs:270-288
    pub fn deduplicate(&self) -> anyhow::Result<DashSet<Uuid>> {
        let cap = unsafe { ffi::zh_index_count(self.hip.0) } as usize + 1;
        let (mut out, mut n) = (vec![0u64; cap], 0usize);
        check(unsafe { ffi::zh_index_deduplicate(self.hip.0, out.as_mut_ptr(), cap, &mut n) })?;
        let t = self.ids.read().unwrap();
        Ok(out[..n.min(cap)].iter().map(|r| t.of_row[*r as usize]).collect())
    }

    /// (new) zh_index_compact: the device memory of removed vectors is reclaimed in place.  The library renumbers its rows (stable: live
    /// rows keep their order) and returns old row -> new row; the row <-> Uuid table is rewritten with it, so Uuids never change and every
    /// later call answers as before.  Removed vectors' Uuids leave the table.  Needs the exclusion of `add`.
    pub fn compact(&self) -> anyhow::Result<ffi::zh_compact_info> {
        let mut t = self.ids.write().unwrap(); // rows are renumbered: hold the table across the call
        let n = unsafe { ffi::zh_index_stored_rows(self.hip.0) } as usize;
        let mut new_ids = vec![u64::MAX; n];
        let mut info = unsafe { std::mem::zeroed::<ffi::zh_compact_info>() };
        check(unsafe { ffi::zh_index_compact(self.hip.0, new_ids.as_mut_ptr(), n, &mut info) })?;
        let mut of_row = Vec::with_capacity(info.rows_after as usize);
        let mut row_of = HashMap::with_capacity(info.rows_after as usize);
        for (old, new) in new_ids.iter().enumerate() {
            if *new != u64::MAX {
                debug_assert_eq!(*new as usize, of_row.len()); // the map is strictly increasing on live rows (id_base is 0 here)
                row_of.insert(t.of_row[old], *new);
                of_row.push(t.of_row[old]);
            }
        }
        t.of_row = of_row;
        t.row_of = row_of;
        Ok(info)
    }

    /// lsh.rs:506-529
    pub fn clear(&self) -> anyhow::Result<()> {
        let mut t = self.ids.write().unwrap();
        t.of_row.clear();
        t.row_of.clear();
        check(unsafe { ffi::zh_index_clear(self.hip.0) })
    }
}

/// The model side of `Database<N, Met, Mod>` (src/model/core.rs:12-37) is untouched by this path; a marker stands in.
pub trait DatabaseEmbeddingModel<const N: usize> {}

/// `Database<N, Met, Mod>` (src/database/core.rs:55-62) for the two calls on the hot path.  In the reference the
/// struct also carries the header (`DatabaseInner`) and a path, and documents live in lz4 files
/// (`save_documents_to_disk` / `read_documents_from_disk`, core.rs:322-380): unchanged code, represented here by an
/// in-memory map so that the skeleton is self-contained.
#[derive(Clone)]
pub struct Database<
    const N: usize,
    Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Default + Send + Sync,
    Mod: DatabaseEmbeddingModel<N> + Default + Send + Sync,
> {
    metric: Met,
    #[allow(dead_code)]
    model: Mod,
    /// The database index used to approximate nearest-neighbour search (pub field, core.rs:62).
    pub index: LSHIndex<N>,
    documents: Arc<DashMap<Uuid, Vec<u8>>>,
}

impl<
        const N: usize,
        Met: Metric<Embedding<N>, Unit = DistanceUnit> + HipMetric + Default + Send + Sync,
        Mod: DatabaseEmbeddingModel<N> + Default + Send + Sync,
    > Database<N, Met, Mod>
{
    pub fn new(uuid: &Uuid, index_options: &LSHIndexOptions<N>) -> anyhow::Result<Self> {
        Ok(Self { metric: Met::default(), model: Mod::default(), index: LSHIndex::new(uuid, index_options)?, documents: Default::default() })
    }

    /// core.rs:245-254
    pub fn insert_records(&self, embeddings: &Vec<Embedding<N>>, documents: &Vec<Vec<u8>>) -> anyhow::Result<()> {
        let embedding_ids = self.index.add(embeddings)?;
        for (id, doc) in embedding_ids.iter().zip(documents) {
            self.documents.insert(*id, doc.clone());
        }
        Ok(())
    }

    /// (new) every record whose key is <= `max_key` for each query (LSHIndex::search_range_batch): query index -> its records, nearest first
    pub fn query_vectors_within(&self, vectors: &Vec<Embedding<N>>, max_key: DistanceUnit) -> anyhow::Result<Vec<Vec<(Uuid, Vec<u8>)>>> {
        if self.index.no_vectors() {
            return Ok(Vec::new());
        }
        let hits = self.index.search_range_batch(vectors, &vec![max_key; vectors.len()], &self.metric)?;
        Ok(hits.into_iter().map(|h| h.into_iter().map(|(id, _)| (id, self.documents.get(&id).map(|d| d.clone()).unwrap_or_default())).collect()).collect())
    }

    /// core.rs:290-313: the rayon loop over queries (core.rs:299-303) is ONE batched call; order and distances are
    /// dropped as in core.rs:304-305.  A batch has no per-query failure mode, so a library error is returned, not
    /// turned into empty entries (the reference's `unwrap_or_default` is per query).
    pub fn query_vectors(&self, vectors: &Vec<Embedding<N>>, number_of_results: usize) -> anyhow::Result<DashMap<usize, DashMap<Uuid, Vec<u8>>>> {
        if self.index.no_vectors() {
            return Ok(DashMap::new()); // core.rs:295-297
        }
        let results = DashMap::new();
        for (idx, neighbours) in self.index.search_batch(vectors, number_of_results, &self.metric)?.into_iter().enumerate() {
            let docs = DashMap::new();
            for (id, _) in neighbours {
                docs.insert(id, self.documents.get(&id).map(|d| d.clone()).unwrap_or_default());
            }
            results.insert(idx, docs);
        }
        Ok(results)
    }

    /// (new) reclaim the device memory of removed vectors; documents are keyed by Uuid and stay as they are
    pub fn compact(&self) -> anyhow::Result<()> {
        self.index.compact().map(|_| ())
    }

    /// core.rs:205-214
    pub fn remove(&self, embedding_ids: &Vec<Uuid>) -> anyhow::Result<()> {
        for id in self.index.remove(embedding_ids)?.iter() {
            self.documents.remove(&*id);
        }
        Ok(())
    }
}
