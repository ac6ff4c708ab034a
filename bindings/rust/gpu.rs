//! `src/gpu.rs` for bliss-rs (`bliss-audio` 0.13.0): the per-song analysis hot path and the feature-vector distances on
//! an MI355X through `libblissgpu.so` (C ABI: `include/blissgpu.h`).  Enabled by a `gpu` cargo feature; the CPU path stays
//! behind `#[cfg(not(feature = "gpu"))]`.
//!
//! **UNTESTED SOURCE**: the image this repository is built in has no `rustc` / `cargo`, so this file has never been
//! compiled.  It binds exactly the symbols that the two tested host layers bind -- `bliss-rs_amd/csrc/bliss_audio.hpp`
//! (C++17, `tests/cpp/test_bliss_audio.cpp`) and `bliss-rs_amd/_ffi.py` (ctypes; `__graft_entry__.build()` checks its
//! signature table against the header and the built library) -- and the declarations below are a line-by-line
//! transcription of `include/blissgpu.h`.
//!
//! What it replaces in the crate (file:line of bliss-rs at the commit under /root/reference):
//!   * `Song::analyze_with_options`            src/song/mod.rs:403-508     -> [`analyze_with_options`]
//!   * the compute half of `Decoder::analyze_paths_with_options`
//!                                             src/song/decoder.rs:278-332 -> [`analyze_decoded`] (one device batch), or the
//!     crate's own worker threads calling [`analyze_with_options`]: concurrent calls are coalesced inside the library and
//!     spread over every GPU of the node
//!   * `FFmpegDecoder::resample_frame` (libswresample to mono 22 050 Hz f32)
//!                                             src/song/decoder/ffmpeg.rs:36-109 -> [`analyze_native`] / [`DecodedPcm`]: the
//!     decoder hands over the codec's own frames, the conversion runs on the device, bit for bit
//!   * `PreAnalyzedSong::to_song_with_options` src/song/decoder.rs:85-101  -> unchanged, it calls `Song::analyze_with_options`
//!   * `euclidean_distance` / `cosine_distance` / `mahalanobis_distance`
//!                                             src/playlist.rs:65-79,140-142 -> [`distance`], [`pairwise`]
//!   * `closest_to_songs` / `song_to_song`     src/playlist.rs:256-326     -> [`order_on_device`]
//!   * `dedup_playlist` / `dedup_playlist_custom_distance`
//!                                             src/playlist.rs:343-402     -> [`dedup_on_device`]
//!   * `closest_to_songs(&[song], ..)` cut after k, many songs per call (`Library::playlist_from(..).take(k)`)
//!                                             src/playlist.rs:256-270     -> [`nearest_on_device`]
//!   * `closest_to_songs(.., &ForestOptions)`  src/playlist.rs:230-270     -> [`forest_order_on_device`]
//!   * the same per album, in one call                                     -> [`forest_group_playlists_on_device`]
//!
//! build.rs of the crate, under the feature:
//! ```ignore
//! if std::env::var("CARGO_FEATURE_GPU").is_ok() {
//!     let dir = std::env::var("BLISSGPU_LIB_DIR").expect("BLISSGPU_LIB_DIR = directory of libblissgpu.so");
//!     println!("cargo:rustc-link-search=native={dir}");
//!     println!("cargo:rustc-link-lib=dylib=blissgpu");
//! }
//! ```
#![cfg(feature = "gpu")]
#![allow(non_camel_case_types)]

use crate::{Analysis, AnalysisOptions, BlissError, BlissResult, FeaturesVersion, Song};
use ndarray::Array2;
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

/// Raw declarations (`include/blissgpu.h`).
pub mod sys {
    use std::os::raw::{c_char, c_int, c_void};

    #[repr(C)]
    pub struct blissgpu_ctx {
        _private: [u8; 0],
    }
    #[repr(C)]
    pub struct blissgpu_node {
        _private: [u8; 0],
    }

    pub const BLISSGPU_OK: c_int = 0;
    pub const BLISSGPU_ERR_NO_DEVICE: c_int = 1;
    pub const BLISSGPU_ERR_INVALID: c_int = 2;
    pub const BLISSGPU_ERR_HIP: c_int = 3;
    pub const BLISSGPU_ERR_OOM: c_int = 4;
    pub const BLISSGPU_ERR_NAN: c_int = 5;
    pub const BLISSGPU_ERR_RCCL: c_int = 6;
    pub const BLISSGPU_ERR_TIMEOUT: c_int = 7;
    pub const BLISSGPU_ERR_INTERNAL: c_int = 8;
    pub const BLISSGPU_SONG_OK: i32 = 0;
    pub const BLISSGPU_SONG_TOO_SHORT: i32 = 1;
    pub const BLISSGPU_SONG_DECODE_ERROR: i32 = 2;
    pub const BLISSGPU_FLAC_INFO_WORDS: usize = 12;
    pub const BLISSGPU_FLAC_CHECK_CRC16: u32 = 1;
    pub const BLISSGPU_FLAC_CHECK_MD5: u32 = 2;
    pub const BLISSGPU_FLAC_BAD_STREAM: u32 = 1;
    pub const BLISSGPU_FLAC_BAD_CRC16: u32 = 2;
    pub const BLISSGPU_FLAC_BAD_MD5: u32 = 4;
    pub const BLISSGPU_FLAC_MD5_UNCHECKED: u32 = 8;
    pub const BLISSGPU_METRIC_EUCLIDEAN: c_int = 0;
    pub const BLISSGPU_METRIC_COSINE: c_int = 1;
    pub const BLISSGPU_METRIC_MAHALANOBIS: c_int = 2;
    pub const BLISSGPU_RADIO_MAX_RULES: u32 = 4;
    pub const BLISSGPU_RADIO_CHAIN: c_int = 0;
    pub const BLISSGPU_RADIO_NEAREST: c_int = 1;
    pub const BLISSGPU_SAMPLE_F32: c_int = 0;
    pub const BLISSGPU_SAMPLE_S16: c_int = 1;
    pub const BLISSGPU_SAMPLE_S32: c_int = 2;
    pub const BLISSGPU_SAMPLE_RATE: u32 = 22050;
    /// the pinned staging ring of the host PCM feed (a `Vec<f32>` is pageable memory): worker threads, 0 = off
    pub const BLISSGPU_OPT_STAGE_LANES: c_int = 9;
    pub const BLISSGPU_OPT_STAGE_SLAB_KIB: c_int = 10;
    pub const BLISSGPU_OPT_STAGE_SLABS: c_int = 11;
    pub const BLISSGPU_OPT_STAGE_NUMA: c_int = 12;

    /// One song as the decoder delivers it (host memory): `frames` frames of `channels` interleaved samples.
    #[repr(C)]
    #[derive(Clone, Copy)]
    pub struct blissgpu_decoded_song {
        pub pcm: *const c_void,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u16,
        pub sample_format: u16,
    }

    extern "C" {
        // ---- contexts ----
        pub fn blissgpu_ctx_create(device: c_int, ctx: *mut *mut blissgpu_ctx) -> c_int;
        pub fn blissgpu_ctx_destroy(ctx: *mut blissgpu_ctx) -> c_int;
        pub fn blissgpu_ctx_synchronize(ctx: *mut blissgpu_ctx) -> c_int;
        pub fn blissgpu_ctx_set_workspace_limit(ctx: *mut blissgpu_ctx, bytes: u64) -> c_int;
        pub fn blissgpu_default_device_count() -> c_int;
        pub fn blissgpu_default_device(k: c_int) -> c_int;
        pub fn blissgpu_default_device_batches(k: c_int) -> u64;
        pub fn blissgpu_default_ctx(k: c_int, ctx: *mut *mut blissgpu_ctx) -> c_int;
        pub fn blissgpu_ctx_set_option(ctx: *mut blissgpu_ctx, option: c_int, value: i64) -> c_int;
        pub fn blissgpu_ctx_staged_bytes(ctx: *mut blissgpu_ctx) -> u64;
        pub fn blissgpu_set_single_song_timeout_ms(ms: i64) -> c_int;
        pub fn blissgpu_feature_count(features_version: u32) -> u32;
        pub fn blissgpu_feature_weights(features_version: u32, out: *mut f32) -> c_int;

        // ---- Song::analyze ----
        pub fn blissgpu_analyze(pcm: *const f32, len: u64, features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_analyze_interleaved(pcm: *const c_void, sample_format: c_int, channels: u32, frames: u64,
                                            features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_analyze_batch(pcm: *const f32, offsets: *const u64, lengths: *const u64, n_songs: u32,
                                      features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_analyze_batch_s16(pcm: *const i16, offsets: *const u64, lengths: *const u64, n_songs: u32,
                                          features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_analyze_batch_interleaved(pcm: *const c_void, sample_format: c_int, channels: u32,
                                                  offsets: *const u64, lengths: *const u64, n_songs: u32,
                                                  features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_analyze_decoded(pcm: *const c_void, sample_format: c_int, channels: u32, frames: u64, sample_rate: u32,
                                        features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_analyze_batch_decoded(songs: *const blissgpu_decoded_song, n_songs: u32, features_version: u32,
                                              out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_resampled_len(frames: u64, sample_rate: u32) -> u64;
        pub fn blissgpu_default_reset() -> c_int;
        pub fn blissgpu_analyze_batch_device(ctx: *mut blissgpu_ctx, d_pcm: *const f32, offsets: *const u64,
                                             lengths: *const u64, n_songs: u32, features_version: u32, d_out: *mut f32,
                                             d_status: *mut i32) -> c_int;

        // ---- distances, playlist ordering ----
        pub fn blissgpu_distance(a: *const f32, b: *const f32, d: u32, metric: c_int, m_matrix: *const f32, out: *mut f32) -> c_int;
        pub fn blissgpu_pairwise(a: *const f32, n: u64, b: *const f32, m: u64, d: u32, metric: c_int, m_matrix: *const f32,
                                 out: *mut f32) -> c_int;
        pub fn blissgpu_set_distance(seeds: *const f32, n_seeds: u32, cand: *const f32, n: u64, d: u32, metric: c_int,
                                     m_matrix: *const f32, out: *mut f32) -> c_int;
        pub fn blissgpu_closest_to_songs(seeds: *const f32, n_seeds: u32, cand: *const f32, n: u64, d: u32, metric: c_int,
                                         m_matrix: *const f32, order: *mut u32, dist: *mut f32) -> c_int;
        pub fn blissgpu_song_to_song(seeds: *const f32, n_seeds: u32, cand: *const f32, n: u64, d: u32, metric: c_int,
                                     m_matrix: *const f32, order: *mut u32) -> c_int;
        pub fn blissgpu_dedup_playlist(x: *const f32, n: u64, d: u32, seq: *const u32, len: u64, meta: *const u32, metric: c_int,
                                       m_matrix: *const f32, threshold: f32, kept: *mut u32, n_kept: *mut u64) -> c_int;
        pub fn blissgpu_dedup_playlist_device(ctx: *mut blissgpu_ctx, d_x: *const f32, n: u64, d: u32, d_seq: *const u32,
                                              len: u64, d_meta: *const u32, metric: c_int, d_m: *const f32, threshold: f32,
                                              d_kept: *mut u32, d_n_kept: *mut u64) -> c_int;
        pub fn blissgpu_knn(queries: *const f32, q: u64, cand: *const f32, n: u64, d: u32, metric: c_int, m_matrix: *const f32,
                            skip: *const u32, k: u32, idx: *mut u32, dist: *mut f32) -> c_int;
        pub fn blissgpu_knn_device(ctx: *mut blissgpu_ctx, d_queries: *const f32, q: u64, d_cand: *const f32, n: u64, d: u32,
                                   metric: c_int, d_m: *const f32, d_skip: *const u32, k: u32, d_idx: *mut u32,
                                   d_dist: *mut f32) -> c_int;
        // the same selection under dist / sqrt(qscale[i] * cscale[j]) (local scaling against hubs), and the k-occurrence counts
        pub fn blissgpu_scaled_knn(queries: *const f32, q: u64, qscale: *const f32, cand: *const f32, n: u64, cscale: *const f32,
                                   d: u32, metric: c_int, m_matrix: *const f32, skip: *const u32, k: u32, idx: *mut u32,
                                   dist: *mut f32) -> c_int;
        pub fn blissgpu_scaled_knn_device(ctx: *mut blissgpu_ctx, d_queries: *const f32, q: u64, d_qscale: *const f32,
                                          d_cand: *const f32, n: u64, d_cscale: *const f32, d: u32, metric: c_int, d_m: *const f32,
                                          d_skip: *const u32, k: u32, d_idx: *mut u32, d_dist: *mut f32) -> c_int;
        pub fn blissgpu_knn_occurrence(idx: *const u32, q: u64, k: u32, n: u64, count: *mut u32) -> c_int;
        pub fn blissgpu_knn_occurrence_device(ctx: *mut blissgpu_ctx, d_idx: *const u32, q: u64, k: u32, n: u64,
                                              d_count: *mut u32) -> c_int;
        // radio playlists: song-to-song chains (mode 0) or the k nearest songs (mode 1) under artist / album separation rules
        pub fn blissgpu_radio(from: *const f32, n_radios: u64, cand: *const f32, n: u64, d: u32, metric: c_int, m_matrix: *const f32,
                              labels: *const u32, from_labels: *const u32, n_rules: u32, window: *const u32, limit: *const u32,
                              skip: *const u32, k: u32, mode: c_int, idx: *mut u32, dist: *mut f32) -> c_int;
        pub fn blissgpu_radio_device(ctx: *mut blissgpu_ctx, d_from: *const f32, n_radios: u64, d_cand: *const f32, n: u64, d: u32,
                                     metric: c_int, d_m: *const f32, d_labels: *const u32, d_from_labels: *const u32, n_rules: u32,
                                     window: *const u32, limit: *const u32, d_skip: *const u32, k: u32, mode: c_int,
                                     d_idx: *mut u32, d_dist: *mut f32) -> c_int;
        pub fn blissgpu_group_knn(seeds: *const f32, group_offsets: *const u64, n_groups: u64, cand: *const f32, n: u64, d: u32,
                                  metric: c_int, m_matrix: *const f32, skip: *const u32, k: u32, idx: *mut u32, dist: *mut f32) -> c_int;
        pub fn blissgpu_group_knn_device(ctx: *mut blissgpu_ctx, d_seeds: *const f32, group_offsets: *const u64, n_groups: u64,
                                         d_cand: *const f32, n: u64, d: u32, metric: c_int, d_m: *const f32, d_skip: *const u32, k: u32,
                                         d_idx: *mut u32, d_dist: *mut f32) -> c_int;
        // the t nearest groups of a labelling per queried group under the average nearest-member distance ("similar artists")
        pub fn blissgpu_group_neighbours(x: *const f32, n: u64, d: u32, labels: *const u32, k: u32, metric: c_int, m_matrix: *const f32,
                                         queries: *const u32, q: u64, t: u32, mode: c_int, slab_groups: u32, idx: *mut u32,
                                         dist: *mut f64, sizes: *mut u32, matrix: *mut f64) -> c_int;
        pub fn blissgpu_group_neighbours_device(ctx: *mut blissgpu_ctx, d_x: *const f32, n: u64, d: u32, d_labels: *const u32, k: u32,
                                                metric: c_int, d_m: *const f32, d_queries: *const u32, q: u64, t: u32, mode: c_int,
                                                slab_groups: u32, d_idx: *mut u32, d_dist: *mut f64, d_sizes: *mut u32,
                                                d_matrix: *mut f64) -> c_int;
        // the minimum spanning tree of a library under (weight bits, lower song, higher song): clusters without k, a tour
        pub fn blissgpu_mst(x: *const f32, n: u64, d: u32, metric: c_int, m_matrix: *const f32, core: *const f32, edge_u: *mut u32,
                            edge_v: *mut u32, edge_w: *mut f32, rounds: *mut u32) -> c_int;
        pub fn blissgpu_mst_device(ctx: *mut blissgpu_ctx, d_x: *const f32, n: u64, d: u32, metric: c_int, d_m: *const f32,
                                   d_core: *const f32, d_edge_u: *mut u32, d_edge_v: *mut u32, d_edge_w: *mut f32,
                                   rounds: *mut u32) -> c_int;
        // one diagonal metric per seed group: variance_based_weight_matrix of every group, and the search under it
        pub fn blissgpu_group_weights(seeds: *const f32, group_offsets: *const u64, n_groups: u64, d: u32, weights: *mut f32,
                                      group_status: *mut i32) -> c_int;
        pub fn blissgpu_group_weights_device(ctx: *mut blissgpu_ctx, d_seeds: *const f32, group_offsets: *const u64, n_groups: u64,
                                             d: u32, d_weights: *mut f32, d_group_status: *mut i32) -> c_int;
        pub fn blissgpu_group_knn_weighted(seeds: *const f32, group_offsets: *const u64, n_groups: u64, cand: *const f32, n: u64,
                                           d: u32, weights: *const f32, skip: *const u32, k: u32, idx: *mut u32, dist: *mut f32,
                                           group_status: *mut i32) -> c_int;
        pub fn blissgpu_group_knn_weighted_device(ctx: *mut blissgpu_ctx, d_seeds: *const f32, group_offsets: *const u64,
                                                  n_groups: u64, d_cand: *const f32, n: u64, d: u32, d_weights: *const f32,
                                                  d_skip: *const u32, k: u32, d_idx: *mut u32, d_dist: *mut f32,
                                                  d_group_status: *mut i32) -> c_int;
        // the k nearest ALBUMS of every seed group: closest_album_to_group cut after k albums
        pub fn blissgpu_album_knn(seeds: *const f32, group_offsets: *const u64, n_groups: u64, cand: *const f32, n: u64, d: u32,
                                  album_of: *const u32, n_albums: u64, skip: *const u32, k: u32, idx: *mut u32, dist: *mut f32,
                                  group_means: *mut f32, centroids: *mut f32) -> c_int;
        pub fn blissgpu_album_knn_device(ctx: *mut blissgpu_ctx, d_seeds: *const f32, group_offsets: *const u64, n_groups: u64,
                                         d_cand: *const f32, n: u64, d: u32, d_album_of: *const u32, n_albums: u64,
                                         d_skip: *const u32, k: u32, d_idx: *mut u32, d_dist: *mut f32, d_group_means: *mut f32,
                                         d_centroids: *mut f32) -> c_int;
        pub fn blissgpu_duplicate_groups(x: *const f32, n: u64, d: u32, meta: *const u32, metric: c_int, m_matrix: *const f32,
                                         threshold: f32, label: *mut u32, n_pairs: *mut u64, pairs: *mut u32, pair_dist: *mut f32,
                                         max_pairs: u64) -> c_int;
        pub fn blissgpu_duplicate_groups_device(ctx: *mut blissgpu_ctx, d_x: *const f32, n: u64, d: u32, d_meta: *const u32,
                                                metric: c_int, d_m: *const f32, threshold: f32, d_label: *mut u32,
                                                d_n_pairs: *mut u64, d_pairs: *mut u32, d_pair_dist: *mut f32,
                                                max_pairs: u64) -> c_int;

        // ---- extended isolation forest (ForestOptions, src/playlist.rs:230-251) ----
        pub fn blissgpu_forest_build(seeds: *const f32, n_seeds: u64, d: u32, n_trees: u32, sample_size: u32, max_tree_depth: u32,
                                     extension_level: u32, seed: u64, forest: *mut *mut c_void) -> c_int;
        pub fn blissgpu_forest_destroy(forest: *mut c_void) -> c_int;
        pub fn blissgpu_forest_info(forest: *const c_void, d: *mut u32, n_trees: *mut u32, psi: *mut u32, depth_limit: *mut u32,
                                    extension_level: *mut u32, n_nodes: *mut u64) -> c_int;
        pub fn blissgpu_forest_export(forest: *const c_void, sample_idx: *mut u32, tree_first: *mut u64, normal: *mut f32,
                                      b: *mut f32, left: *mut u32, right: *mut u32, leaf_size: *mut u32, leaf_q: *mut u32) -> c_int;
        pub fn blissgpu_forest_score(forest: *mut c_void, cand: *const f32, n: u64, score: *mut f32, path_sum: *mut u64) -> c_int;
        pub fn blissgpu_forest_closest_to_songs(forest: *mut c_void, cand: *const f32, n: u64, order: *mut u32,
                                                score: *mut f32) -> c_int;
        pub fn blissgpu_forest_score_device(ctx: *mut blissgpu_ctx, forest: *mut c_void, d_cand: *const f32, n: u64,
                                            d_score: *mut f32, d_path_sum: *mut u64) -> c_int;
        pub fn blissgpu_forest_closest_to_songs_device(ctx: *mut blissgpu_ctx, forest: *mut c_void, d_cand: *const f32, n: u64,
                                                       d_order: *mut u32, d_score: *mut f32) -> c_int;
        // one forest per seed group: the k lowest forest scores of every group in one call
        pub fn blissgpu_group_forest_knn(seeds: *const f32, group_offsets: *const u64, n_groups: u64, cand: *const f32, n: u64, d: u32,
                                         n_trees: u32, sample_size: u32, max_tree_depth: u32, extension_level: u32, seed: u64,
                                         skip: *const u32, k: u32, idx: *mut u32, score: *mut f32, group_status: *mut i32) -> c_int;
        pub fn blissgpu_group_forest_knn_device(ctx: *mut blissgpu_ctx, d_seeds: *const f32, h_seeds: *const f32,
                                                group_offsets: *const u64, n_groups: u64, d_cand: *const f32, n: u64, d: u32,
                                                n_trees: u32, sample_size: u32, max_tree_depth: u32, extension_level: u32, seed: u64,
                                                d_skip: *const u32, k: u32, d_idx: *mut u32, d_score: *mut f32,
                                                d_group_status: *mut i32) -> c_int;
        pub fn blissgpu_group_forest_plan(group_offsets: *const u64, n_groups: u64, d: u32, n_trees: u32, sample_size: u32,
                                          max_tree_depth: u32, extension_level: u32, node_budget: u64, batch_first: *mut u64,
                                          max_batches: u64, n_batches: *mut u64) -> c_int;
        pub fn blissgpu_debug_group_forest_stats(ctx: *mut blissgpu_ctx, build_ms: *mut f64, wait_ms: *mut f64, n_batches: *mut u64) -> c_int;

        // ---- one process, every GPU of the node ----
        pub fn blissgpu_node_create(n_devices: c_int, devices: *const c_int, node: *mut *mut blissgpu_node) -> c_int;
        pub fn blissgpu_node_destroy(node: *mut blissgpu_node) -> c_int;
        pub fn blissgpu_node_analyze(node: *mut blissgpu_node, pcm: *const f32, offsets: *const u64, lengths: *const u64,
                                     n_songs: u32, features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_node_pairwise(node: *mut blissgpu_node, metric: c_int, m_matrix: *const f32, out: *mut f32) -> c_int;
        pub fn blissgpu_node_synchronize(node: *mut blissgpu_node) -> c_int;
        pub fn blissgpu_shard_plan(lengths: *const u64, n_songs: u32, world: u32, rank_of_song: *mut u32) -> c_int;

        // ---- page-locked decode buffers (full PCIe rate) ----
        pub fn blissgpu_host_alloc(h_ptr: *mut *mut c_void, bytes: u64) -> c_int;
        pub fn blissgpu_host_free(h_ptr: *mut c_void) -> c_int;

        pub fn blissgpu_strerror(code: c_int) -> *const c_char;
        // FLAC decoded on the device: compressed files in, PCM / feature rows out
        pub fn blissgpu_flac_info(file: *const c_void, nbytes: u64, info: *mut u64) -> c_int;
        pub fn blissgpu_flac_index(file: *const c_void, nbytes: u64, verified: c_int, info: *mut u64, frames: *mut u64, max_frames: u64, n_frames: *mut u64) -> c_int;
        pub fn blissgpu_flac_decode_device(ctx: *mut blissgpu_ctx, d_bytes: *const c_void, nbytes: u64, frames: *const u64, n_frames: u64, info: *const u64, d_pcm: *mut c_void, d_frame_status: *mut i32, d_frame_end: *mut u64) -> c_int;
        pub fn blissgpu_flac_decode(file: *const c_void, nbytes: u64, pcm: *mut c_void, max_bytes: u64, info: *mut u64, status: *mut i32) -> c_int;
        pub fn blissgpu_flac_decode_batch(files: *mut *const c_void, nbytes: *const u64, n_songs: u32, pcm: *mut *mut c_void, max_bytes: *const u64, info: *mut u64, status: *mut i32) -> c_int;
        pub fn blissgpu_analyze_batch_flac(files: *mut *const c_void, nbytes: *const u64, n_songs: u32, features_version: u32, out: *mut f32, status: *mut i32) -> c_int;
        pub fn blissgpu_ctx_flac_slow_songs(ctx: *mut blissgpu_ctx) -> u64;
        // FLAC verified on the device: frame CRC-16 and stream MD5, a verdict per song
        pub fn blissgpu_flac_verify_batch(files: *mut *const c_void, nbytes: *const u64, n_songs: u32, checks: u32, flags: *mut u32, first_bad_frame: *mut u32, md5: *mut c_void) -> c_int;
        pub fn blissgpu_analyze_batch_flac_verified(files: *mut *const c_void, nbytes: *const u64, n_songs: u32, features_version: u32, checks: u32, out: *mut f32, status: *mut i32, flags: *mut u32, first_bad_frame: *mut u32) -> c_int;
        pub fn blissgpu_flac_crc16_device(ctx: *mut blissgpu_ctx, d_bytes: *const c_void, nbytes: u64, frames: *const u64, n_frames: u64, d_frame_status: *const i32, d_frame_end: *const u64, d_frame_crc_ok: *mut i32) -> c_int;
        pub fn blissgpu_flac_md5_device(ctx: *mut blissgpu_ctx, d_pcm: *const c_void, info: *const u64, d_md5: *mut c_void) -> c_int;
        // acoustic fingerprints (Haitsma & Kalker) and their match over candidate pairs
        pub fn blissgpu_fingerprint_len(n_samples: u64) -> u64;
        pub fn blissgpu_fingerprint_bands(edges: *mut u32) -> c_int;
        pub fn blissgpu_fingerprint_batch(pcm: *const f32, sample_offsets: *const u64, word_offsets: *const u64, n_songs: u32, words: *mut u32, status: *mut i32, energies: *mut f64) -> c_int;
        pub fn blissgpu_fingerprint_match(words: *const u32, word_offsets: *const u64, n_songs: u32, pairs: *const u32, n_pairs: u64, max_offset: u32, min_overlap: u32, offset: *mut i32, errors: *mut u32, bits: *mut u32) -> c_int;
        // loudness (EBU R 128 / ReplayGain 2.0): the device-free tables and gates, the device's energies and peaks, the whole batch
        pub fn blissgpu_loudness_subblocks(frames: u64, sample_rate: u32) -> u64;
        pub fn blissgpu_loudness_kweighting(sample_rate: u32, coef: *mut f64) -> c_int;
        pub fn blissgpu_true_peak_filter(sample_rate: u32, factor: *mut u32, h: *mut f64) -> c_int;
        pub fn blissgpu_loudness_blocks(z: *const f64, channels: u32, n_sub: u64, sample_rate: u32, p: *mut f64, st: *mut f64) -> c_int;
        pub fn blissgpu_loudness_gate(p: *const f64, n: u64, power: *mut f64, lufs: *mut f64) -> c_int;
        pub fn blissgpu_loudness_range(st: *const f64, n: u64, range_lu: *mut f64, lo: *mut f64, hi: *mut f64) -> c_int;
        pub fn blissgpu_loudness_energies(songs: *const blissgpu_decoded_song, n_songs: u32, z: *mut f64, sample_peak: *mut f64, true_peak: *mut f64, status: *mut i32) -> c_int;
        pub fn blissgpu_loudness_batch(songs: *const blissgpu_decoded_song, n_songs: u32, album: *const u32, n_albums: u32, song_out: *mut f64, album_out: *mut f64, status: *mut i32) -> c_int;
        pub fn blissgpu_last_error() -> *const c_char;
        pub fn blissgpu_version() -> *const c_char;
    }
}

fn last_error() -> String {
    let p: *const c_char = unsafe { sys::blissgpu_last_error() };
    if p.is_null() {
        return String::new();
    }
    unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned()
}

/// A failed call never crosses the boundary as a panic: whole-call return code + per-song status.
fn gpu_err(rc: c_int) -> BlissError {
    match rc {
        sys::BLISSGPU_ERR_NO_DEVICE => BlissError::ProviderError(format!("no usable MI355X for libblissgpu (there is no CPU fallback): {}", last_error())),
        _ => BlissError::AnalysisError(format!("blissgpu error {rc}: {}", last_error())),
    }
}

fn too_short() -> BlissError {
    // src/song/mod.rs:426-430
    BlissError::AnalysisError(String::from("empty or too short song."))
}

fn version_code(v: FeaturesVersion) -> u32 {
    v as u16 as u32 // FeaturesVersion::Version1 = 1, Version2 = 2 (src/lib.rs:151-160)
}

/// Same contract as the CPU `Song::analyze_with_options` (src/song/mod.rs:413-508): mono 22 050 Hz f32 samples in,
/// `Analysis` out, `AnalysisError("empty or too short song.")` below 8192 samples.  Called from the crate's
/// `number_cores` worker threads (src/song/decoder.rs:299-329) it keeps every GPU of the node busy: the library coalesces
/// concurrent calls into device batches, one default context per visible device.
pub fn analyze_with_options(sample_array: &[f32], analysis_options: &AnalysisOptions) -> BlissResult<Analysis> {
    let version = analysis_options.features_version;
    let mut out = vec![0f32; version.feature_count()];
    let mut status = 0i32;
    let rc = unsafe {
        sys::blissgpu_analyze(sample_array.as_ptr(), sample_array.len() as u64, version_code(version), out.as_mut_ptr(), &mut status)
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    if status == sys::BLISSGPU_SONG_TOO_SHORT {
        return Err(too_short());
    }
    Analysis::new(out, version)
}

impl Song {
    /// Drop-in for the CPU associated function of the same name when the `gpu` feature is on.
    pub fn analyze_with_options_gpu(sample_array: &[f32], analysis_options: &AnalysisOptions) -> BlissResult<Analysis> {
        analyze_with_options(sample_array, analysis_options)
    }
}

/// Bulk form for `Decoder::analyze_paths_with_options`: decode on the CPU workers as today, then hand the decoded buffers
/// over in ONE call instead of analysing per thread (src/song/decoder.rs:304-328).  The library orders the songs by
/// length, cuts them into chunks that fit its workspace and streams the PCM over PCIe group by group -- straight from
/// the callers' buffers: nothing is copied on the host.
pub fn analyze_decoded(songs: &[&[f32]], version: FeaturesVersion) -> BlissResult<Vec<BlissResult<Analysis>>> {
    let native: Vec<DecodedPcm> = songs.iter().map(|s| DecodedPcm::F32 { samples: s, channels: 1, sample_rate: sys::BLISSGPU_SAMPLE_RATE }).collect();
    analyze_native(&native, version)
}

/// What a decoder delivers BEFORE the conversion `FFmpegDecoder::resample_frame` does (src/song/decoder/ffmpeg.rs:36-109):
/// interleaved frames at the file's own rate.  The library converts to mono 22 050 Hz f32 on the device exactly as
/// libswresample does with the decoder's options -- same filter, same summation order; the reference's Adler-32 decoder
/// tests (ffmpeg.rs:433-452) hold for its output -- so a decoder built on this skips `resample_frame` altogether.
#[derive(Clone, Copy)]
pub enum DecodedPcm<'a> {
    F32 { samples: &'a [f32], channels: u16, sample_rate: u32 },
    S16 { samples: &'a [i16], channels: u16, sample_rate: u32 },
    /// FFmpeg's AV_SAMPLE_FMT_S32 (24-bit streams arrive left-justified)
    S32 { samples: &'a [i32], channels: u16, sample_rate: u32 },
}

impl<'a> DecodedPcm<'a> {
    fn raw(&self) -> sys::blissgpu_decoded_song {
        let (pcm, len, channels, sample_rate, fmt) = match *self {
            DecodedPcm::F32 { samples, channels, sample_rate } => (samples.as_ptr() as *const c_void, samples.len(), channels, sample_rate, sys::BLISSGPU_SAMPLE_F32),
            DecodedPcm::S16 { samples, channels, sample_rate } => (samples.as_ptr() as *const c_void, samples.len(), channels, sample_rate, sys::BLISSGPU_SAMPLE_S16),
            DecodedPcm::S32 { samples, channels, sample_rate } => (samples.as_ptr() as *const c_void, samples.len(), channels, sample_rate, sys::BLISSGPU_SAMPLE_S32),
        };
        sys::blissgpu_decoded_song { pcm, frames: (len / channels.max(1) as usize) as u64, sample_rate, channels, sample_format: fmt as u16 }
    }
    /// Samples at 22 050 Hz this song becomes (`PreAnalyzedSong::duration`, src/song/decoder.rs:34-65).
    pub fn resampled_len(&self) -> u64 {
        let r = self.raw();
        unsafe { sys::blissgpu_resampled_len(r.frames, r.sample_rate) }
    }
}

/// `analyze_paths_with_options` for decoders that keep the file's format: a library of 44.1 / 48 kHz, mono / stereo, 16 /
/// 24-bit files in one call (blissgpu_analyze_batch_decoded).
pub fn analyze_native(songs: &[DecodedPcm], version: FeaturesVersion) -> BlissResult<Vec<BlissResult<Analysis>>> {
    let d = version.feature_count();
    let raw: Vec<sys::blissgpu_decoded_song> = songs.iter().map(|s| s.raw()).collect();
    let mut out = vec![0f32; songs.len() * d];
    let mut status = vec![0i32; songs.len()];
    let rc = unsafe { sys::blissgpu_analyze_batch_decoded(raw.as_ptr(), raw.len() as u32, version_code(version), out.as_mut_ptr(), status.as_mut_ptr()) };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(status
        .iter()
        .enumerate()
        .map(|(i, &st)| if st == sys::BLISSGPU_SONG_TOO_SHORT { Err(too_short()) } else { Analysis::new(out[i * d..(i + 1) * d].to_vec(), version) })
        .collect())
}

/// The three metrics the library evaluates (bit for bit like src/playlist.rs:65-79,140-142, ndarray's summation order
/// included).  Custom closures and the isolation-forest metric stay on the CPU iterators.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Metric {
    Euclidean,
    Cosine,
    Mahalanobis,
}

impl Metric {
    fn code(self) -> c_int {
        match self {
            Metric::Euclidean => sys::BLISSGPU_METRIC_EUCLIDEAN,
            Metric::Cosine => sys::BLISSGPU_METRIC_COSINE,
            Metric::Mahalanobis => sys::BLISSGPU_METRIC_MAHALANOBIS,
        }
    }
}

fn matrix_ptr(m: Option<&Array2<f32>>) -> (Option<Array2<f32>>, *const f32) {
    let owned = m.map(|m| m.as_standard_layout().to_owned());
    let p = owned.as_ref().map_or(std::ptr::null(), |m| m.as_ptr());
    (owned, p)
}

/// One pair (`Analysis::distance` / `Song::distance`, src/song/mod.rs:364-370,519-521): one kernel launch.
pub fn distance(a: &[f32], b: &[f32], metric: Metric, m: Option<&Array2<f32>>) -> BlissResult<f32> {
    assert_eq!(a.len(), b.len());
    let (_keep, mp) = matrix_ptr(m);
    let mut out = 0f32;
    let rc = unsafe { sys::blissgpu_distance(a.as_ptr(), b.as_ptr(), a.len() as u32, metric.code(), mp, &mut out) };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(out)
}

/// All pairs between the rows of `a` and the rows of `b` (row-major `n x d` / `m x d`), `n x m` out.
pub fn pairwise(a: &Array2<f32>, b: &Array2<f32>, metric: Metric, m: Option<&Array2<f32>>) -> BlissResult<Array2<f32>> {
    assert_eq!(a.ncols(), b.ncols());
    let (a, b) = (a.as_standard_layout(), b.as_standard_layout());
    let (_keep, mp) = matrix_ptr(m);
    let mut out = vec![0f32; a.nrows() * b.nrows()];
    let rc = unsafe {
        sys::blissgpu_pairwise(a.as_ptr(), a.nrows() as u64, b.as_ptr(), b.nrows() as u64, a.ncols() as u32, metric.code(), mp, out.as_mut_ptr())
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(Array2::from_shape_vec((a.nrows(), b.nrows()), out).expect("n x m"))
}

/// `closest_to_songs` (src/playlist.rs:256-270; `chain = false`: stable sort by the summed distance to the seed set) and
/// `song_to_song` (:272-326; `chain = true`: greedy nearest-neighbour chain) for the built-in metrics: the same order as
/// the CPU iterators, ties included; only the permutation comes back from the device.  A NaN distance is
/// `BLISSGPU_ERR_NAN` here where `n32()` / `argmin().unwrap()` panic on the CPU path.
pub fn order_on_device<T: AsRef<Song> + Clone>(initial: &[T], candidates: &[T], metric: Metric, m: Option<&Array2<f32>>,
                                               chain: bool) -> BlissResult<Vec<T>> {
    let d = candidates.first().map_or(0, |s| s.as_ref().analysis.as_vec().len());
    let flat = |songs: &[T]| songs.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let (seeds, cand) = (flat(initial), flat(candidates));
    let (_keep, mp) = matrix_ptr(m);
    let mut order = vec![0u32; candidates.len()];
    let rc = unsafe {
        if chain {
            sys::blissgpu_song_to_song(seeds.as_ptr(), initial.len() as u32, cand.as_ptr(), candidates.len() as u64, d as u32,
                                       metric.code(), mp, order.as_mut_ptr())
        } else {
            sys::blissgpu_closest_to_songs(seeds.as_ptr(), initial.len() as u32, cand.as_ptr(), candidates.len() as u64, d as u32,
                                           metric.code(), mp, order.as_mut_ptr(), std::ptr::null_mut())
        }
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(order.into_iter().map(|i| candidates[i as usize].clone()).collect())
}

/// `dedup_playlist_custom_distance` (src/playlist.rs:367-402) for the built-in metrics in one library call: a song absorbs
/// the songs that follow it while they are closer than `distance_threshold` (default 0.05) or carry the same `Some` title
/// and artist.  A NaN distance the CPU iterator would evaluate is `BLISSGPU_ERR_NAN` here where `n32()` panics.
pub fn dedup_on_device<T: AsRef<Song> + Clone>(playlist: &[T], distance_threshold: Option<f32>, metric: Metric,
                                               m: Option<&Array2<f32>>) -> BlissResult<Vec<T>> {
    if playlist.is_empty() {
        return Ok(Vec::new());
    }
    let d = playlist[0].as_ref().analysis.as_vec().len();
    let x = playlist.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    // one key per song: 0 when the title or the artist is None, equal keys for equal (title, artist)
    let mut seen = std::collections::HashMap::new();
    let meta = playlist
        .iter()
        .map(|s| match (&s.as_ref().title, &s.as_ref().artist) {
            (Some(t), Some(a)) => {
                let next = seen.len() as u32 + 1;
                *seen.entry((t.clone(), a.clone())).or_insert(next)
            }
            _ => 0,
        })
        .collect::<Vec<u32>>();
    let (_keep, mp) = matrix_ptr(m);
    let mut kept = vec![0u32; playlist.len()];
    let mut n_kept = 0u64;
    let rc = unsafe {
        sys::blissgpu_dedup_playlist(x.as_ptr(), playlist.len() as u64, d as u32, std::ptr::null(), playlist.len() as u64,
                                     meta.as_ptr(), metric.code(), mp, distance_threshold.unwrap_or(0.05), kept.as_mut_ptr(),
                                     &mut n_kept)
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(kept[..n_kept as usize].iter().map(|&i| playlist[i as usize].clone()).collect())
}

/// `closest_to_songs(&[song], candidates, metric)` cut after `k` (src/playlist.rs:256-270) for every song of `songs` in one
/// library call -- what `Library::playlist_from(&[song])?.take(k)` (src/library.rs:762-850) asks per song: the `k` nearest
/// candidates in ascending distance, equal distances in candidate order, no distance matrix.  `exclude_self` leaves the
/// first candidate equal to the song (`Song: PartialEq`) out of that song's list.  A NaN distance is `BLISSGPU_ERR_NAN`.
pub fn nearest_on_device<T: AsRef<Song> + Clone>(songs: &[T], candidates: &[T], k: usize, metric: Metric, m: Option<&Array2<f32>>,
                                                 exclude_self: bool) -> BlissResult<Vec<Vec<T>>> {
    if songs.is_empty() || candidates.is_empty() {
        return Ok(vec![Vec::new(); songs.len()]);
    }
    let d = candidates[0].as_ref().analysis.as_vec().len();
    let flat = |songs: &[T]| songs.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let (queries, cand) = (flat(songs), flat(candidates));
    let skip = songs
        .iter()
        .map(|s| if exclude_self { candidates.iter().position(|c| c.as_ref() == s.as_ref()).map_or(u32::MAX, |j| j as u32) } else { u32::MAX })
        .collect::<Vec<u32>>();
    let (_keep, mp) = matrix_ptr(m);
    let mut idx = vec![0u32; songs.len() * k];
    let rc = unsafe {
        sys::blissgpu_knn(queries.as_ptr(), songs.len() as u64, cand.as_ptr(), candidates.len() as u64, d as u32, metric.code(), mp,
                          skip.as_ptr(), k as u32, idx.as_mut_ptr(), std::ptr::null_mut())
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(idx.chunks(k).map(|row| row.iter().filter(|&&j| j != u32::MAX).map(|&j| candidates[j as usize].clone()).collect()).collect())
}

/// `closest_to_songs(group, candidates without the group's songs, metric)` cut after `k` (src/playlist.rs:36-59, 256-270) for
/// every group of `groups` in one library call -- what `Library::playlist_from(&[several songs])?.take(k)`
/// (src/library.rs:762-842) asks per album, artist or saved playlist: a candidate's score is the sequential sum of its
/// distances to the group's songs, in their order; equal scores come in candidate order.  `exclude_members` leaves the first
/// candidate equal to each member (`Song: PartialEq`) out of that group's list.  A NaN score is `BLISSGPU_ERR_NAN`.
pub fn group_playlists_on_device<T: AsRef<Song> + Clone>(groups: &[Vec<T>], candidates: &[T], k: usize, metric: Metric,
                                                         m: Option<&Array2<f32>>, exclude_members: bool) -> BlissResult<Vec<Vec<T>>> {
    if groups.is_empty() || candidates.is_empty() {
        return Ok(vec![Vec::new(); groups.len()]);
    }
    let d = candidates[0].as_ref().analysis.as_vec().len();
    let cand = candidates.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let seeds = groups.iter().flatten().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let mut offsets = vec![0u64; groups.len() + 1];
    for (g, group) in groups.iter().enumerate() {
        offsets[g + 1] = offsets[g] + group.len() as u64;
    }
    let skip = groups
        .iter()
        .flatten()
        .map(|s| if exclude_members { candidates.iter().position(|c| c.as_ref() == s.as_ref()).map_or(u32::MAX, |j| j as u32) } else { u32::MAX })
        .collect::<Vec<u32>>();
    let (_keep, mp) = matrix_ptr(m);
    let mut idx = vec![0u32; groups.len() * k];
    let rc = unsafe {
        sys::blissgpu_group_knn(seeds.as_ptr(), offsets.as_ptr(), groups.len() as u64, cand.as_ptr(), candidates.len() as u64, d as u32,
                                metric.code(), mp, skip.as_ptr(), k as u32, idx.as_mut_ptr(), std::ptr::null_mut())
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(idx.chunks(k).map(|row| row.iter().filter(|&&j| j != u32::MAX).map(|&j| candidates[j as usize].clone()).collect()).collect())
}

/// `closest_album_to_group(group, pool)` (src/playlist.rs:424-485) cut after the `number_albums` closest albums, for every
/// group of `groups` in one library call -- what `Library::album_playlist_from` (src/library.rs:850-893) asks per album: the
/// group, then each chosen album's pool songs by (disc, track) number.  Albums are numbered in order of first appearance in
/// `pool`; the first pool song equal to each member (`Song: PartialEq`) leaves the pool before its album's mean is formed;
/// equal distances come in order of first appearance.  A NaN distance is `BLISSGPU_ERR_NAN`, an empty group
/// `BLISSGPU_ERR_INVALID` (the reference's "Mean of empty slice").
pub fn album_playlists_on_device<T: AsRef<Song> + Clone>(groups: &[Vec<T>], pool: &[T], number_albums: usize) -> BlissResult<Vec<Vec<T>>> {
    let mut names: Vec<&str> = Vec::new();
    let album_of = pool
        .iter()
        .map(|s| match s.as_ref().album.as_deref() {
            None => u32::MAX,
            Some(a) => names.iter().position(|&b| b == a).unwrap_or_else(|| { names.push(a); names.len() - 1 }) as u32,
        })
        .collect::<Vec<u32>>();
    let k = number_albums.min(names.len());
    if groups.is_empty() || k == 0 {
        return Ok(groups.to_vec());
    }
    let d = pool[0].as_ref().analysis.as_vec().len();
    let cand = pool.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let seeds = groups.iter().flatten().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let mut offsets = vec![0u64; groups.len() + 1];
    for (g, group) in groups.iter().enumerate() {
        offsets[g + 1] = offsets[g] + group.len() as u64;
    }
    let skip = groups
        .iter()
        .flatten()
        .map(|s| pool.iter().position(|c| c.as_ref() == s.as_ref()).map_or(u32::MAX, |j| j as u32))
        .collect::<Vec<u32>>();
    let mut idx = vec![0u32; groups.len() * k];
    let rc = unsafe {
        sys::blissgpu_album_knn(seeds.as_ptr(), offsets.as_ptr(), groups.len() as u64, cand.as_ptr(), pool.len() as u64, d as u32,
                                album_of.as_ptr(), names.len() as u64, skip.as_ptr(), k as u32, idx.as_mut_ptr(), std::ptr::null_mut(),
                                std::ptr::null_mut(), std::ptr::null_mut())
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(groups
        .iter()
        .enumerate()
        .map(|(g, group)| {
            let gone = &skip[offsets[g] as usize..offsets[g + 1] as usize];
            let mut playlist = group.clone();
            for &a in idx[g * k..(g + 1) * k].iter().filter(|&&a| a != u32::MAX) {
                let mut album = (0..pool.len()).filter(|&i| album_of[i] == a && !gone.contains(&(i as u32))).collect::<Vec<usize>>();
                album.sort_by_key(|&i| (pool[i].as_ref().disc_number, pool[i].as_ref().track_number));
                playlist.extend(album.into_iter().map(|i| pool[i].clone()));
            }
            playlist
        })
        .collect())
}

/// The duplicate rule of `dedup_playlist_custom_distance` (src/playlist.rs:381-388) over EVERY pair of `songs`, closed
/// transitively: the groups of two or more songs that are closer than `distance_threshold` (default 0.05) or carry the same
/// `Some` title and artist, directly or through a chain of such pairs.  Groups come by their first member, members in the
/// order of `songs`; one library call, no distance matrix.  A NaN distance is `BLISSGPU_ERR_NAN`.
pub fn duplicate_groups_on_device<T: AsRef<Song> + Clone>(songs: &[T], distance_threshold: Option<f32>, metric: Metric,
                                                          m: Option<&Array2<f32>>) -> BlissResult<Vec<Vec<T>>> {
    if songs.is_empty() {
        return Ok(Vec::new());
    }
    let d = songs[0].as_ref().analysis.as_vec().len();
    let x = songs.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let mut seen = std::collections::HashMap::new();
    let meta = songs
        .iter()
        .map(|s| match (&s.as_ref().title, &s.as_ref().artist) {
            (Some(t), Some(a)) => {
                let next = seen.len() as u32 + 1;
                *seen.entry((t.clone(), a.clone())).or_insert(next)
            }
            _ => 0,
        })
        .collect::<Vec<u32>>();
    let (_keep, mp) = matrix_ptr(m);
    let mut label = vec![0u32; songs.len()];
    let mut n_pairs = 0u64;
    let rc = unsafe {
        sys::blissgpu_duplicate_groups(x.as_ptr(), songs.len() as u64, d as u32, meta.as_ptr(), metric.code(), mp,
                                       distance_threshold.unwrap_or(0.05), label.as_mut_ptr(), &mut n_pairs, std::ptr::null_mut(),
                                       std::ptr::null_mut(), 0)
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    // a label is its group's smallest row: walking the rows in order yields groups by first member, members ascending
    let mut groups = std::collections::BTreeMap::<u32, Vec<T>>::new();
    for (i, s) in songs.iter().enumerate() {
        groups.entry(label[i]).or_default().push(s.clone());
    }
    Ok(groups.into_values().filter(|g| g.len() >= 2).collect())
}

/// `ForestOptions` of the CPU crate (src/playlist.rs:230-251) plus the 64-bit seed that makes the forest reproducible:
/// the same (seed songs, options, seed) give the same forest and therefore the same playlist.
#[derive(Clone, Copy, Debug)]
pub struct ForestOptions {
    pub n_trees: usize,
    pub sample_size: usize,
    pub max_tree_depth: Option<usize>,
    pub extension_level: usize,
    pub seed: u64,
}

/// `closest_to_songs(initial, candidates, &ForestOptions)` (src/playlist.rs:256-270 with the metric of :230-251): the forest is
/// built on the host from the initial songs (at least two: the forest does not work for a single song), every candidate is
/// scored on the device and the stable order of the scores comes back.  Scores are always finite: no `BLISSGPU_ERR_NAN` here.
pub fn forest_order_on_device<T: AsRef<Song> + Clone>(initial: &[T], candidates: &[T], options: &ForestOptions) -> BlissResult<Vec<T>> {
    if candidates.is_empty() {
        return Ok(Vec::new());
    }
    let d = candidates[0].as_ref().analysis.as_vec().len();
    let flat = |songs: &[T]| songs.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let (seeds, cand) = (flat(initial), flat(candidates));
    let mut forest: *mut c_void = std::ptr::null_mut();
    let rc = unsafe {
        sys::blissgpu_forest_build(seeds.as_ptr(), initial.len() as u64, d as u32, options.n_trees as u32, options.sample_size.min(u32::MAX as usize) as u32,
                                   options.max_tree_depth.map_or(0, |k| k.max(1).min(u32::MAX as usize) as u32), options.extension_level as u32,
                                   options.seed, &mut forest)
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    let mut order = vec![0u32; candidates.len()];
    let rc = unsafe { sys::blissgpu_forest_closest_to_songs(forest, cand.as_ptr(), candidates.len() as u64, order.as_mut_ptr(), std::ptr::null_mut()) };
    unsafe { sys::blissgpu_forest_destroy(forest) };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(order.into_iter().map(|i| candidates[i as usize].clone()).collect())
}

/// `closest_to_songs(group, candidates without the group's songs, &ForestOptions)` cut after `k` for every group of `groups`
/// in one library call: one forest per group (same options, same seed), built on the host while the device scores the
/// previous ones.  A group with `min(sample_size, members) < 2` has no forest and gets an empty list.
pub fn forest_group_playlists_on_device<T: AsRef<Song> + Clone>(groups: &[Vec<T>], candidates: &[T], k: usize, options: &ForestOptions,
                                                                exclude_members: bool) -> BlissResult<Vec<Vec<T>>> {
    if groups.is_empty() || candidates.is_empty() {
        return Ok(vec![Vec::new(); groups.len()]);
    }
    let d = candidates[0].as_ref().analysis.as_vec().len();
    let cand = candidates.iter().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let seeds = groups.iter().flatten().flat_map(|s| s.as_ref().analysis.as_vec()).collect::<Vec<f32>>();
    let mut offsets = vec![0u64; groups.len() + 1];
    for (g, group) in groups.iter().enumerate() {
        offsets[g + 1] = offsets[g] + group.len() as u64;
    }
    let skip = groups
        .iter()
        .flatten()
        .map(|s| if exclude_members { candidates.iter().position(|c| c.as_ref() == s.as_ref()).map_or(u32::MAX, |j| j as u32) } else { u32::MAX })
        .collect::<Vec<u32>>();
    let mut idx = vec![0u32; groups.len() * k];
    let rc = unsafe {
        sys::blissgpu_group_forest_knn(seeds.as_ptr(), offsets.as_ptr(), groups.len() as u64, cand.as_ptr(), candidates.len() as u64,
                                       d as u32, options.n_trees as u32, options.sample_size.min(u32::MAX as usize) as u32,
                                       options.max_tree_depth.map_or(0, |k| k.max(1).min(u32::MAX as usize) as u32),
                                       options.extension_level as u32, options.seed, skip.as_ptr(), k as u32, idx.as_mut_ptr(),
                                       std::ptr::null_mut(), std::ptr::null_mut())
    };
    if rc != sys::BLISSGPU_OK {
        return Err(gpu_err(rc));
    }
    Ok(idx.chunks(k).map(|row| row.iter().filter(|&&j| j != u32::MAX).map(|&j| candidates[j as usize].clone()).collect()).collect())
}

/// One process driving every GPU of the node: songs sharded by sample count, one `ncclAllGather` of the feature rows over
/// xGMI, row-block-sharded pairwise distances.  (The worker-thread pattern above needs none of this.)
pub struct Node {
    raw: *mut sys::blissgpu_node,
    n_songs: usize,
}

// the library serialises per context and is re-entrant; the handle may move between threads
unsafe impl Send for Node {}

impl Node {
    /// `devices = None`: HIP devices 0 .. n_devices.
    pub fn new(n_devices: usize, devices: Option<&[c_int]>) -> BlissResult<Node> {
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { sys::blissgpu_node_create(n_devices as c_int, devices.map_or(std::ptr::null(), |d| d.as_ptr()), &mut raw) };
        if rc != sys::BLISSGPU_OK {
            return Err(gpu_err(rc));
        }
        Ok(Node { raw, n_songs: 0 })
    }

    /// Analyses `songs` across the node; afterwards every device holds the full `n x d` matrix.
    pub fn analyze(&mut self, songs: &[&[f32]], version: FeaturesVersion) -> BlissResult<Vec<BlissResult<Analysis>>> {
        let d = version.feature_count();
        let lengths: Vec<u64> = songs.iter().map(|s| s.len() as u64).collect();
        let mut offsets = Vec::with_capacity(songs.len());
        let mut pcm: Vec<f32> = Vec::new();
        for s in songs {
            offsets.push(pcm.len() as u64);
            pcm.extend_from_slice(s);
        }
        let mut out = vec![0f32; songs.len() * d];
        let mut status = vec![0i32; songs.len()];
        let rc = unsafe {
            sys::blissgpu_node_analyze(self.raw, pcm.as_ptr(), offsets.as_ptr(), lengths.as_ptr(), songs.len() as u32, version_code(version),
                                       out.as_mut_ptr(), status.as_mut_ptr())
        };
        if rc != sys::BLISSGPU_OK {
            return Err(gpu_err(rc));
        }
        self.n_songs = songs.len();
        Ok(status
            .iter()
            .enumerate()
            .map(|(i, &st)| if st == sys::BLISSGPU_SONG_TOO_SHORT { Err(too_short()) } else { Analysis::new(out[i * d..(i + 1) * d].to_vec(), version) })
            .collect())
    }

    /// All-pairs distances over the gathered matrix, one row block per device.
    pub fn pairwise(&mut self, metric: Metric, m: Option<&Array2<f32>>) -> BlissResult<Array2<f32>> {
        let (_keep, mp) = matrix_ptr(m);
        let n = self.n_songs;
        let mut out = vec![0f32; n * n];
        let rc = unsafe { sys::blissgpu_node_pairwise(self.raw, metric.code(), mp, out.as_mut_ptr()) };
        if rc != sys::BLISSGPU_OK {
            return Err(gpu_err(rc));
        }
        Ok(Array2::from_shape_vec((n, n), out).expect("n x n"))
    }
}

impl Drop for Node {
    fn drop(&mut self) {
        unsafe { sys::blissgpu_node_destroy(self.raw) };
    }
}
